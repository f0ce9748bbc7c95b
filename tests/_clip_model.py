"""Host model of the gradient-norm contract of include/upflow_hip.h (upf_grads_sumsq_check, upf_grad_norm_clip_coef): what the
kernels must compute, written from the contract and not from the kernels.

    norm  = sqrt(sum of g^2 over every gradient element) / S          g: the fp32 gradients still multiplied by S
    coef  = float32(min(float64(max_norm) / (float64(float32 norm) + 1e-6), 1))
"""
import math

import numpy as np


def norm64(grads, scale=1.0):
    """The L2 norm of the un-scaled gradients as a python float (fp64): `grads` fp32 arrays / tensors holding S * g.  The square of
    an fp32 value is exact in float64; math.fsum adds the squares without rounding error, so only the square root and the division
    by the power of two S (exact) round."""
    total = []
    for g in grads:
        a = np.asarray(g.detach().cpu().numpy() if hasattr(g, 'detach') else g)
        assert a.dtype == np.float32
        a = a.astype(np.float64).ravel()
        total.append(math.fsum(a * a))
    return math.sqrt(math.fsum(total)) / float(scale)


def coef32(norm, max_norm):
    """The clip coefficient from an fp32 norm, step 3 of the contract: float64 arithmetic, one rounding to float32."""
    n = np.float64(np.float32(norm))
    with np.errstate(over='ignore'):
        c = np.float64(np.float32(max_norm)) / (n + np.float64(1e-6))
    return np.float32(min(c, np.float64(1.0)))


def ulps32(a, b):
    """|a - b| in units of the fp32 spacing at b."""
    b32 = np.float32(b)
    return abs(float(a) - float(b)) / float(np.spacing(np.abs(b32)))
