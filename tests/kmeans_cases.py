"""Shared by tests/test_oracle_golden.py and tests/test_gpu_kmeans.py (not a test module): the C oracle's fp32 k-means step through
ctypes, and the inputs with exact ties that both hold their assignment to."""
import ctypes

import numpy as np


def kmeans_f32(coracle, dense, centers, cnorm=None):
    """oracle_kmeans_assign_f32 (the bit-exact specification of the device's integer step) through ctypes"""
    dense = np.ascontiguousarray(dense, dtype=np.float32)
    centers = np.ascontiguousarray(centers, dtype=np.float32)
    K, D = centers.shape
    if cnorm is None:
        cnorm = np.zeros(K, np.float32)
        coracle.oracle_kmeans_cnorm_f32(centers.ctypes.data_as(ctypes.c_void_p), K, D, cnorm.ctypes.data_as(ctypes.c_void_p))
    units = np.full(len(dense), -1, np.int64)
    coracle.oracle_kmeans_assign_f32(dense.ctypes.data_as(ctypes.c_void_p), len(dense), D, centers.ctypes.data_as(ctypes.c_void_p),
                                     cnorm.ctypes.data_as(ctypes.c_void_p), K, units.ctypes.data_as(ctypes.c_void_p))
    return units


def kmeans_tie_cases(seed=0, K=100, D=768):
    """(dense [T,D], centers [K,D], expected or None): exact ties by construction -- duplicated centroids (identical scores
    bit for bit), centroid pairs that differ only where x is exactly 0 (same dot-product chain, same norm), a NaN row, an Inf row"""
    rs = np.random.RandomState(seed)
    c = rs.standard_normal((K, D)).astype(np.float32)
    x = rs.standard_normal((40, D)).astype(np.float32)
    c[17] = c[5]                    # duplicates: 5 must win whenever either is the minimum
    c[K - 1] = c[60]
    c[31] = c[30]
    c[31, :8] = -c[30, :8]          # differs from 30 only on dims 0..7 -> tie for every x with x[:8] == 0
    x[:, :8] = 0.0
    for t, k in enumerate((5, 17, 60, K - 1, 30, 31)):   # frames sitting ON a member of each tied pair
        x[t] = c[k]
        x[t, :8] = 0.0
    x[20] = np.nan
    x[21] = np.inf
    x[22] = 0.0
    return x, c
