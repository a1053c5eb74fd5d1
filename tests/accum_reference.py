"""TEST INFRASTRUCTURE ONLY -- NumPy models of npm_accumulate_ranges and npm_clip_finish_scaled (include/npm_hip.h) and the bound the
accumulated gradient is held to against the full batch in float64.  Nothing here is measured.

* the fold: float32 ``a + b`` in micro-batch order, one rounding per addition: bit for bit;
* the sum of squares of the folded buffers: ``adamw_reference.exact_sumsq``, the model npm_sumsq_ranges itself is held to (the fused
  sum has no bound of its own: it must be the BITS of npm_sumsq_ranges of the same library on the updated buffers);
* the scaled clip factor: the header's expression in fp64, every operation rounded on its own, one rounding to float32: bit for bit;
* the full batch: with G_j the float64 gradient of micro-batch j's summed loss and g_j what the device made of it, elementwise

      |s sum_j g_j (folded in float32) - s sum_j G_j|  <=  s (sum_j P(G_j) + (k - 1) 2^-24 sum_j |g_j|),     s = grad_scale

  P(G) = NPM_PARITY_SCALED_F32 max |G|, the project's parity contract for one gradient tensor in its elementwise form (the
  relative part of the contract, NPM_PARITY_REL_F32 on elements of at least 0.1 max |G|, is never the smaller one there:
  1e-4 x 0.1 max |G| = 1e-5 max |G|); each of the k - 1 float32 additions errs by at most 2^-24 of its own result, which is at most
  sum_j |g_j|."""

import numpy as np

from adamw_reference import TILE, exact_sumsq  # noqa: F401  (the sum every test of the fold compares with)


def fold(grads):
    """The float32 sum of ``grads`` in order: the first is adopted, every later one added with one rounding."""
    acc = np.array(grads[0], dtype=np.float32, copy=True)
    with np.errstate(all='ignore'):
        for g in grads[1:]:
            acc = acc + np.asarray(g, dtype=np.float32)
    return acc


def clip_finish_scaled(sumsq: float, max_norm: float, grad_scale: float):
    """(norm, scale, ok) as doubles."""
    with np.errstate(all='ignore'):
        s = np.float64(grad_scale)
        norm = s * np.sqrt(np.float64(sumsq))
        if not np.isfinite(norm):
            return float(norm), 0.0, 0.0
        ratio = np.float64(max_norm) / (norm + np.float64(1e-6))
        c = ratio if ratio < 1.0 else np.float64(1.0)
        return float(norm), float(np.float32(s * c)), 1.0


def parity_bound(reference64, scaled_bound: float) -> float:
    """P(G) of the module docstring: one number for every element of the tensor."""
    reference64 = np.asarray(reference64, dtype=np.float64)
    return scaled_bound * float(np.abs(reference64).max()) if reference64.size else 0.0


def full_batch_bound(references64, micro_grads32, grad_scale: float, scaled_bound: float) -> np.ndarray:
    """The elementwise bound of the module docstring for ONE parameter: its k float64 micro-gradients and its k device ones."""
    k = len(references64)
    magnitude = sum(np.abs(np.asarray(g, dtype=np.float64)) for g in micro_grads32)
    return grad_scale * (sum(parity_bound(G, scaled_bound) for G in references64) + (k - 1) * 2.0 ** -24 * magnitude)
