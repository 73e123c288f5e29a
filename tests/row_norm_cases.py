"""Cases and the plain reference of the row-normalisation kernels (K6, on-policy_amd/csrc/mappo_norm.hip), shared by
tests/test_row_norm_cpu.py and tests/test_gpu_row_norm.py.

* the width table: for every ``(VEC, LPR, EPL)`` of ``LN_FOR_SHAPES`` two widths or more that ``pick_shape`` sends
  there (the ends of the shape's range, or the widths the networks use), for operands on 16-byte boundaries (``ALIGNED``: VEC 4), for widths that are no multiple of
  four (``SCALAR``: VEC 1) and for multiples of four with an operand off a 16-byte boundary (``MISALIGNED``: demoted to
  VEC 1);
* ``row_counts``: one row, one row more than a workgroup covers per trip, and the smallest count past the grid cap whose
  second trip ends ragged;
* ``reference``: ``y, mean, rstd, dx, dw, db, dpre_bias`` of ``y = LayerNorm(act(x + pre_bias))`` from the defining
  formulas, in the dtype asked for -- float64 is the yardstick, float32 on the device "the same expression in torch".
"""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM_SOURCE = os.path.join(ROOT, "on-policy_amd", "csrc", "mappo_norm.hip")
THREADS = 256                       # kThreads of mappo_norm.hip: a workgroup covers THREADS / LPR rows per trip
EPS = 1e-5

ALIGNED = (12, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 512, 516, 1024, 1028, 2048)
SCALAR = (1, 2, 3, 5, 7, 11, 14, 17, 21, 33, 42, 65, 127, 129, 150, 257, 435, 513, 1023, 1025, 1285, 1535)
MISALIGNED = (64, 512, 1024, 1536)
# (width, aligned16) of every case of the table
TABLE = tuple((D, 1) for D in ALIGNED + SCALAR) + tuple((D, 0) for D in MISALIGNED)
REFUSED = ((1537, 1), (2052, 1), (2049, 1), (2048, 0))


def built_shapes():
    """The ``(VEC, LPR, EPL)`` list of ``LN_FOR_SHAPES``, parsed out of the kernel source."""
    src = open(NORM_SOURCE).read()
    body = re.search(r"#define LN_FOR_SHAPES\(X\)((?:.*\\\n)*.*)\n", src).group(1)
    return [tuple(int(v) for v in m) for m in re.findall(r"X\((\d+),\s*(\d+),\s*(\d+)\)", body)]


def decode(code):
    """``mappo_layernorm_shape``'s value -> (vec, lpr, epl), or None for a refused width."""
    return None if code == 0 else (code & 255, (code >> 8) & 255, code >> 16)


def shape_of(lib, D, aligned16=1):
    return decode(lib.mappo_layernorm_shape(D, aligned16))


def row_counts(lpr, cap):
    rpb = THREADS // lpr
    return (1, rpb + 1, cap * rpb + rpb // 2 + 1)


def activation(z, act):
    """act 0 / 1 / 2 = identity / tanh / relu -> (value, derivative); relu'(0) = 0 as in torch and in the kernels."""
    if act == 1:
        a = torch.tanh(z)
        return a, 1 - a * a
    if act == 2:
        on = (z > 0).to(z.dtype)
        return z * on, on
    return z, torch.ones_like(z)


def reference(x, pre_bias, weight, bias, dy, act, dtype=torch.float64, eps=EPS):
    """-> dict(y, mean, rstd, dx, dw, db, dpre, scale_dw, scale_db, scale_dpre, scale_mean) in ``dtype``.

    The pre-activation is the FLOAT32 sum x + pre_bias, promoted: both precisions then see the same number, so no ReLU unit
    is on in one and off in the other.  ``dx`` is the gradient at the pre-activation, ``dpre`` its column sums; the scales
    are what a sum's error is measured against: the largest column's sum of |per-row term| for the three column sums, the
    largest row's mean of |activation| for ``mean`` (a row's mean may cancel to nothing)."""
    z = (x if pre_bias is None else x + pre_bias).to(dtype)
    w, b, g_out = weight.to(dtype), bias.to(dtype), dy.to(dtype)
    a, da = activation(z, act)
    D = z.shape[-1]
    mean = a.sum(-1, keepdim=True) / D
    c = a - mean
    rstd = 1.0 / torch.sqrt((c * c).sum(-1, keepdim=True) / D + eps)
    xhat = c * rstd
    y = xhat * w + b
    g = g_out * w
    m1 = g.sum(-1, keepdim=True) / D
    m2 = (g * xhat).sum(-1, keepdim=True) / D
    dx = rstd * (g - m1 - xhat * m2) * da
    tw = g_out * xhat
    return dict(y=y, mean=mean.reshape(-1), rstd=rstd.reshape(-1), dx=dx, dw=tw.sum(0), db=g_out.sum(0), dpre=dx.sum(0),
                scale_dw=tw.abs().sum(0).max(), scale_db=g_out.abs().sum(0).max(), scale_dpre=dx.abs().sum(0).max(),
                scale_mean=(a.abs().sum(-1) / D).max())


def standardized(x, dtype=torch.float64, eps=EPS):
    """(x - mean) / sqrt(var + eps) per row, biased variance: the parameter-free half of the input LayerNorm."""
    x = x.to(dtype)
    D = x.shape[-1]
    c = x - x.sum(-1, keepdim=True) / D
    return c / torch.sqrt((c * c).sum(-1, keepdim=True) / D + eps)


def make_inputs(rows, D, device, seed=0, far=False, relu_zeros=False, with_pre=True):
    """Seeded float32 inputs on ``device``: x = 3 randn + 1 (``far``: 100 + randn, where a one-pass variance has lost its
    digits), LayerNorm weight / bias away from (1, 0), a pre-bias, an upstream gradient.  ``relu_zeros``: 1 % of the
    entries sit at x = -pre_bias exactly (ReLU's kink; at x = 0 and ``pre`` None without ``with_pre``)."""
    g = torch.Generator(device=device).manual_seed(1000003 * seed + 4099 * D + rows)
    rnd = lambda *s: torch.randn(*s, device=device, generator=g)
    x = 100.0 + rnd(rows, D) if far else 3.0 * rnd(rows, D) + 1.0
    pre = 0.5 * rnd(D) + 0.25
    if relu_zeros:
        kink = torch.rand(rows, D, device=device, generator=g) < 0.01
        x = torch.where(kink, (-pre if with_pre else torch.zeros_like(pre)).expand(rows, D), x)
    weight = 1.5 + 0.5 * rnd(D)
    bias = 0.3 * rnd(D) - 0.7
    dy = rnd(rows, D)
    return dict(x=x.contiguous(), pre=pre if with_pre else None, weight=weight, bias=bias, dy=dy)
