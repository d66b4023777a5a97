// torch.optim.AdamW (amsgrad False, maximize False, decoupled decay; its non-capturable single-tensor path) over every leaf of an
// optimiser in ONE launch of up to 16 tensors.  The update reads p, g, m, v and writes p, m, v: 28 B per element, nothing else to
// do, so the kernel is a stream.  The pointers, counts and per-tensor scalars travel by value in the kernel's arguments (no
// per-step upload); workgroups take fixed chunks of ADAMW_CHUNK elements and find their tensor by a wave-uniform scan of the
// table.  No atomics, every element written by one thread, no contraction of a multiply into an add: a tensor's bits depend on
// (p, g, m, v, the scalars) alone, not on the list it is in nor on whether it took the float4 or the scalar path.
#include <math.h>

#include "common.h"

namespace dissc {

constexpr int ADAMW_MAX_TENSORS = 16;
constexpr int ADAMW_THREADS = 256;
constexpr int ADAMW_CHUNK = 4096;  // elements per workgroup: four float4s (or sixteen scalars) per thread
constexpr long long ADAMW_MAX_CHUNKS = 1ll << 30;

struct AdamwArgs {  // by value, 1 KB
  float* p[ADAMW_MAX_TENSORS];
  const float* g[ADAMW_MAX_TENSORS];
  float* m[ADAMW_MAX_TENSORS];
  float* v[ADAMW_MAX_TENSORS];
  size_t numel[ADAMW_MAX_TENSORS];
  unsigned first[ADAMW_MAX_TENSORS];    // the tensor's first workgroup; strictly increasing, first[0] = 0
  float step_size[ADAMW_MAX_TENSORS];   // lr / (1 - b1^t), t per tensor
  float bc2_sqrt[ADAMW_MAX_TENSORS];    // sqrt(1 - b2^t)
  unsigned vec;                         // bit i: the four pointers of tensor i are 16-byte aligned
  int n;
  float decay, omb1, b2, omb2, eps;     // 1 - lr wd, 1 - b1, b2, 1 - b2, eps: each rounded once from double
};

// one element, in torch's order and with torch's roundings (every product and sum rounded on its own):
//   p *= 1 - lr wd;  m += (g - m)(1 - b1)  [lerp_ at a weight below 0.5, i.e. b1 > 0.5];  v = v b2 + ((1 - b2) g) g  [mul_, addcmul_];
//   denom = sqrt(v) / sqrt(1 - b2^t) + eps;  p -= (lr / (1 - b1^t)) (m / denom)  [addcdiv_]
__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, float decay, float omb1, float b2, float omb2,
                                          float eps, float step_size, float bc2_sqrt) {
#pragma clang fp contract(off)
  const float pd = p * decay;
  const float mi = m + (g - m) * omb1;
  const float vi = v * b2 + (omb2 * g) * g;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  m = mi;
  v = vi;
  p = pd - step_size * (mi / denom);
}

__global__ void __launch_bounds__(ADAMW_THREADS) adamw_kernel(const AdamwArgs a) {
  // wave-uniform scan: the last tensor whose first workgroup is at or below this one (first[0] = 0)
  int ti = 0;
#pragma unroll
  for (int i = 1; i < ADAMW_MAX_TENSORS; ++i)
    if (i < a.n && a.first[i] <= blockIdx.x) ti = i;
  float* __restrict__ p = a.p[ti];
  const float* __restrict__ g = a.g[ti];
  float* __restrict__ m = a.m[ti];
  float* __restrict__ v = a.v[ti];
  const size_t numel = a.numel[ti];
  const float step_size = a.step_size[ti], bc2_sqrt = a.bc2_sqrt[ti];
  const size_t base = (size_t)(blockIdx.x - a.first[ti]) * ADAMW_CHUNK;  // < numel: the tensor has ceil(numel / CHUNK) workgroups
  const int tid = threadIdx.x;
  if ((a.vec >> ti) & 1) {
    // float4 i4 < floor(numel / 4) lies inside the tensor; the last numel % 4 elements go one by one in its last workgroup
    const size_t n4 = numel >> 2;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* m4 = reinterpret_cast<f32x4*>(m);
    f32x4* v4 = reinterpret_cast<f32x4*>(v);
#pragma unroll
    for (int j = 0; j < ADAMW_CHUNK / 4 / ADAMW_THREADS; ++j) {
      const size_t i4 = base / 4 + tid + (size_t)ADAMW_THREADS * j;
      if (i4 < n4) {
        f32x4 pp = p4[i4], mm = m4[i4], vv = v4[i4];
        const f32x4 gg = g4[i4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float pe = pp[e], me = mm[e], ve = vv[e];
          adamw_one(pe, gg[e], me, ve, a.decay, a.omb1, a.b2, a.omb2, a.eps, step_size, bc2_sqrt);
          pp[e] = pe, mm[e] = me, vv[e] = ve;
        }
        p4[i4] = pp, m4[i4] = mm, v4[i4] = vv;
      }
    }
    if (base + ADAMW_CHUNK >= numel && tid < (int)(numel & 3)) {  // 4 n4 + tid < numel
      const size_t i = 4 * n4 + tid;
      adamw_one(p[i], g[i], m[i], v[i], a.decay, a.omb1, a.b2, a.omb2, a.eps, step_size, bc2_sqrt);
    }
  } else {
#pragma unroll 4
    for (int j = 0; j < ADAMW_CHUNK / ADAMW_THREADS; ++j) {
      const size_t i = base + tid + (size_t)ADAMW_THREADS * j;
      if (i < numel) adamw_one(p[i], g[i], m[i], v[i], a.decay, a.omb1, a.b2, a.omb2, a.eps, step_size, bc2_sqrt);
    }
  }
}

}  // namespace dissc

using namespace dissc;

extern "C" {

int dissc_adamw_chunk(void) { return ADAMW_CHUNK; }
int dissc_adamw_max_tensors(void) { return ADAMW_MAX_TENSORS; }

int dissc_adamw_step(int n, float* const* p, const float* const* g, float* const* m, float* const* v, const long long* numel,
                     const long long* t, double lr, double b1, double b2, double eps, double weight_decay, void* stream) {
  if (n < 1 || n > ADAMW_MAX_TENSORS || !p || !g || !m || !v || !numel || !t) {
    set_error("dissc_adamw_step: need 1 .. %d tensors (n = %d) and the six host arrays", ADAMW_MAX_TENSORS, n);
    return DISSC_EINVAL;
  }
  if (!(lr >= 0.0) || !(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0) || !(eps >= 0.0) || !(weight_decay >= 0.0)) {
    set_error("dissc_adamw_step: lr %g, betas (%g, %g), eps %g, weight_decay %g: need lr, eps, weight_decay >= 0 and 0 <= beta < 1",
              lr, b1, b2, eps, weight_decay);
    return DISSC_EINVAL;
  }
  AdamwArgs a;
  a.n = n;
  a.vec = 0;
  a.decay = (float)(1.0 - lr * weight_decay);
  a.omb1 = (float)(1.0 - b1);
  a.b2 = (float)b2;
  a.omb2 = (float)(1.0 - b2);
  a.eps = (float)eps;
  long long chunks = 0;
  for (int i = 0; i < ADAMW_MAX_TENSORS; ++i) {
    if (i >= n) {
      a.p[i] = a.m[i] = a.v[i] = nullptr;
      a.g[i] = nullptr;
      a.numel[i] = 0;
      a.first[i] = 0;
      a.step_size[i] = a.bc2_sqrt[i] = 0.f;
      continue;
    }
    if (!p[i] || !g[i] || !m[i] || !v[i] || numel[i] < 1 || t[i] < 1) {
      set_error("dissc_adamw_step: tensor %d: null pointer, numel %lld below 1 or step %lld below 1", i, numel[i], t[i]);
      return DISSC_EINVAL;
    }
    if (p[i] == m[i] || p[i] == v[i] || m[i] == v[i] || g[i] == p[i] || g[i] == m[i] || g[i] == v[i]) {
      set_error("dissc_adamw_step: tensor %d: p, g, m and v must be four different buffers", i);
      return DISSC_EINVAL;
    }
    a.p[i] = p[i], a.g[i] = g[i], a.m[i] = m[i], a.v[i] = v[i];
    a.numel[i] = (size_t)numel[i];
    a.first[i] = (unsigned)chunks;
    chunks += (numel[i] + ADAMW_CHUNK - 1) / ADAMW_CHUNK;
    if (numel[i] > ADAMW_MAX_CHUNKS * ADAMW_CHUNK || chunks > ADAMW_MAX_CHUNKS) {
      set_error("dissc_adamw_step: more than %lld chunks of %d elements in one launch (at tensor %d)", ADAMW_MAX_CHUNKS, ADAMW_CHUNK, i);
      return DISSC_EINVAL;
    }
    if ((((uintptr_t)p[i] | (uintptr_t)g[i] | (uintptr_t)m[i] | (uintptr_t)v[i]) & 15) == 0) a.vec |= 1u << i;
    const double bc1 = 1.0 - pow(b1, (double)t[i]), bc2 = 1.0 - pow(b2, (double)t[i]);
    a.step_size[i] = (float)(lr / bc1);
    a.bc2_sqrt[i] = (float)sqrt(bc2);
  }
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)chunks), dim3(ADAMW_THREADS), 0, (hipStream_t)stream, a);
  DISSC_HIP_CHECK(hipGetLastError());
  return DISSC_OK;
}

}  // extern "C"
