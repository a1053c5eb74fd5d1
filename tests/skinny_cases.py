"""Cases shared by tests/test_skinny_host.py (host simulator) and tests/test_gpu_skinny.py (MI355X): the grid of the skinny-M
GEMM, its epilogue combinations, a float64 reference and the GEMM calls a decode step makes."""

import numpy as np

LAYOUTS = ('NT', 'NN')
ROWS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 48, 63, 64)
SHAPES = ((16, 16), (48, 32), (272, 528), (1024, 1024), (1536, 1024), (3072, 1024), (4096, 1024), (1024, 4096))   # (N, K)
EPI_BIAS, EPI_RESIDUAL, EPI_RELU_SAVE, EPI_RELU = 1, 2, 4, 16
# what the decode path asks for (bias, bias + residual, bias + ReLU, bias + ReLU with the saved pre-activation), the plain
# product, and a residual without a bias
EPILOGUES = (0, EPI_BIAS, EPI_BIAS | EPI_RESIDUAL, EPI_BIAS | EPI_RELU, EPI_BIAS | EPI_RELU_SAVE, EPI_RESIDUAL)
TOL = 2e-6            # the project's bound for single GEMM kernels (tests/test_gpu_gemm.py)
LAYER_TOL = 1e-5      # decode against forward (tests/test_gpu_decode.py)


def reference(a, b, layout, alpha=1.0, epilogue=0, bias=None, residual=None):
    """(C, pre-activation or None) in float64."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    v = alpha * (a @ (b.T if layout == 'NT' else b))
    if epilogue & EPI_BIAS:
        v = v + np.asarray(bias, dtype=np.float64)
    if epilogue & EPI_RESIDUAL:
        v = v + np.asarray(residual, dtype=np.float64)
    pre = v.copy() if epilogue & EPI_RELU_SAVE else None
    if epilogue & (EPI_RELU | EPI_RELU_SAVE):
        v = np.maximum(v, 0.0)
    return v, pre


def decode_products(features, hidden, heads, kv_heads, rows, packed=True):
    """(layout, m, n, k, epilogue) of the GEMMs of one TransformerDecoder.decode call, in launch order: self-attention
    projections and output, cross-attention query and output, dense1 (ReLU, pre-activation not kept) and dense2."""
    fkv = features // heads * kv_heads
    if packed:
        out = [('NT', rows, features + 2 * fkv, features, EPI_BIAS)]
    else:
        out = [('NT', rows, features, features, EPI_BIAS), ('NT', rows, fkv, features, EPI_BIAS), ('NT', rows, fkv, features, EPI_BIAS)]
    out += [('NT', rows, features, features, EPI_BIAS | EPI_RESIDUAL), ('NT', rows, features, features, EPI_BIAS),
            ('NT', rows, features, features, EPI_BIAS | EPI_RESIDUAL), ('NN', rows, hidden, features, EPI_BIAS | EPI_RELU),
            ('NN', rows, features, hidden, EPI_BIAS | EPI_RESIDUAL)]
    return out
