"""Shared by tests/test_gan_loss_cpu.py and tests/test_gpu_mpd.py (not a test module): torch restatements, in any dtype and under
autograd, of the three GAN losses (reference sr/models.py:352-383) -- first literally, with torch.mean over whole maps, then in the
ragged form dissc_amd.nn.gan_loss computes on PAIRED pre-activation maps [2 R, C, ld] (rows 0 .. R - 1 real, R .. 2 R - 1
generated, row r and row R + r of length lens[r]): only the valid part of a row is ever touched, so whatever lies beyond it -- a
poison value included -- cannot reach a result.  The bars are conv_grad_ref's."""
import torch
import torch.nn.functional as F

from conv_grad_ref import check, compare, k_cap, K_WHOLE, K_CH  # noqa: F401

FM, DISC, GEN = 0, 1, 2  # dissc_amd.nn.FM / DISC / GEN
SLOPE = 0.1              # reference sr/models.py:13
MAX_MAPS = 64            # DISSC_GANLOSS_MAX_MAPS
WG_UNITS = 1024          # float4s per half that one workgroup of the loss kernels takes (include/dissc_hip.h)


# ---- the reference's three functions as it writes them: lists of whole tensors, torch.mean ---------------------------------
def literal_feature_loss(fmap_r, fmap_g):
    """fmap_r / fmap_g: per discriminator a list of ACTIVATED maps"""
    loss = 0
    for dr, dg in zip(fmap_r, fmap_g):
        for rl, gl in zip(dr, dg):
            loss = loss + torch.mean(torch.abs(rl - gl))
    return loss * 2


def literal_discriminator_loss(real_outputs, generated_outputs):
    loss, r_losses, g_losses = 0, [], []
    for dr, dg in zip(real_outputs, generated_outputs):
        r_loss, g_loss = torch.mean((1 - dr) ** 2), torch.mean(dg ** 2)
        loss = loss + (r_loss + g_loss)
        r_losses.append(r_loss)
        g_losses.append(g_loss)
    return loss, r_losses, g_losses


def literal_generator_loss(outputs):
    loss, gen_losses = 0, []
    for dg in outputs:
        l = torch.mean((1 - dg) ** 2)
        gen_losses.append(l)
        loss = loss + l
    return loss, gen_losses


# ---- the ragged form on paired maps ------------------------------------------------------------------------------------------
def valid_halves(x, lens, R):
    """(real, gen): the valid elements of the two halves of a paired map x [2 R, C, ld] as flat tensors (views of x's rows cut
    at their lengths; positions at or beyond a length are never touched)"""
    real = [x[r, :, :int(lens[r])].reshape(-1) for r in range(R) if int(lens[r]) > 0]
    gen = [x[R + r, :, :int(lens[r])].reshape(-1) for r in range(R) if int(lens[r]) > 0]
    if not real:
        return None, None
    return torch.cat(real), torch.cat(gen)


def map_values(op, x, lens, R, slope=1.0):
    """the one or two values of one paired PRE-activation map, as 0-dim tensors of x's dtype (v0, v1); v1 is zero unless DISC.
    N = 0 (no valid element): zeros that depend on nothing."""
    real, gen = valid_halves(x, lens, R)
    zero = torch.zeros((), dtype=x.dtype)
    if real is None:
        return zero, zero
    if op == FM:
        return 2 * torch.mean(torch.abs(F.leaky_relu(real, slope) - F.leaky_relu(gen, slope))), zero
    if op == DISC:
        return torch.mean((1 - real) ** 2), torch.mean(gen ** 2)
    assert op == GEN
    return torch.mean((1 - gen) ** 2), zero


def loss_ref(ops, maps, lens, R, slopes, dtype, g_total=1.0, g_vals=None):
    """nn.gan_loss on the CPU in ``dtype``: (total, vals [2, n], [gradient per map]) of the cotangents g_total (of the total) and
    g_vals [2, n] (of the values; None: zero).  The gradients are zero beyond the lengths: nothing there was ever read."""
    n = len(maps)
    ops = [ops] * n if isinstance(ops, int) else list(ops)
    xs = [m.detach().to("cpu", dtype).requires_grad_(True) for m in maps]
    v0, v1 = [], []
    for op, x, ln, r, s in zip(ops, xs, lens, R, slopes):
        a, b = map_values(op, x, ln, r, s)
        v0.append(a)
        v1.append(b)
    vals = torch.stack([torch.stack(v0), torch.stack(v1)])
    total = torch.zeros((), dtype=dtype)
    for a, b in zip(v0, v1):
        total = total + (a + b)
    seed = total * g_total
    if g_vals is not None:
        seed = seed + (vals * g_vals.detach().to("cpu", dtype)).sum()
    if seed.requires_grad:
        seed.backward()
    grads = [x.grad if x.grad is not None else torch.zeros_like(x) for x in xs]
    return total.detach(), vals.detach(), grads


def beyond_mask(shape, lens, R):
    """boolean [2 R, C, ld]: True at and beyond the rows' lengths"""
    m = torch.ones(shape, dtype=torch.bool)
    for r in range(R):
        m[r, :, :int(lens[r])] = False
        m[R + r, :, :int(lens[r])] = False
    return m


def workspace_bytes(R, C, ld):
    """include/dissc_hip.h: two doubles per workgroup of WG_UNITS float4s per half, rounded up to 256 bytes"""
    wgs = sum(-(-(r * c * (l // 4)) // WG_UNITS) for r, c, l in zip(R, C, ld))
    return (wgs * 16 + 255) // 256 * 256
