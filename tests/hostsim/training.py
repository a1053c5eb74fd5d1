"""TEST INFRASTRUCTURE ONLY -- the entry points of training, restated with NumPy / the oracle / the reference modules of tests/:
GEMM with its epilogues, elementwise and row kernels (layer and RMS normalisation, the gated SiLU), the fused attention core
(grouped and not), rotary embeddings, convolution, Adam and AdamW with the clipping in front of it, losses and dropout."""

import ctypes as C

import numpy as np

import adamw_reference as AR
import llama_reference as LR
import rope_reference as RR
import xent_cases
import xent_reference
from oracle import np_oracle as O

from .memory import BAD, UNSUPPORTED, _addr, _deref, _heads, _ints, _mat, _vec, _words

SUMSQ_MAX_RANGES = 32                     # NPM_SUMSQ_MAX_RANGES


class Training:
    def __init__(self):
        super().__init__()
        self.ropes = []                   # the arguments of every npm_rope
        self.sumsq_tables = []            # [(address, n), ...] of every npm_sumsq_ranges
        self.last_xent = b''

    # ---- GEMM ----------------------------------------------------------------------------
    def npm_sgemm(self, gref):
        self.calls.append('npm_sgemm')
        return self._sgemm(_deref(gref))

    def _sgemm(self, g):
        """The float64 restatement of every GEMM entry point; the caller records the call."""
        sums = np.zeros((g.batch1, g.n), dtype=np.float64)
        for z0 in range(g.batch0):
            for z1 in range(g.batch1):
                oa = 4 * (z0 * g.stride_a0 + z1 * g.stride_a1)
                ob = 4 * (z0 * g.stride_b0 + z1 * g.stride_b1)
                oc = 4 * (z0 * g.stride_c0 + z1 * g.stride_c1)
                a = _mat(g.a + oa, g.k, g.m, g.lda).T if g.trans_a else _mat(g.a + oa, g.m, g.k, g.lda)
                b = _mat(g.b + ob, g.n, g.k, g.ldb).T if g.trans_b else _mat(g.b + ob, g.k, g.n, g.ldb)
                v = np.float64(g.alpha) * (a.astype(np.float64) @ b.astype(np.float64))
                if g.epilogue & 32:
                    z = z0 * g.batch1 + z1
                    v = np.float64(g.alpha) * _mat(g.aux + oc, g.m, g.n, g.ldaux) * (
                        a.astype(np.float64) @ b.astype(np.float64) - _vec(g.rowvec + 4 * z * g.m, g.m).astype(np.float64)[:, None])
                if g.epilogue & 1:
                    v = v + _vec(g.bias, g.n).astype(np.float64)
                if g.epilogue & 2:
                    v = v + _mat(g.residual + oc, g.m, g.n, g.ldr).astype(np.float64)
                if g.epilogue & 4:
                    _mat(g.aux + oc, g.m, g.n, g.ldaux)[:] = v
                    v = np.maximum(v, 0.0)
                if g.epilogue & 8:
                    v = np.where(_mat(g.aux + oc, g.m, g.n, g.ldaux) >= 0, v, 0.0)
                if g.epilogue & 16:
                    v = np.maximum(v, 0.0)
                _mat(g.c + oc, g.m, g.n, g.ldc)[:] = v
                if g.epilogue & 128:                     # NPM_EPI_ROWDOT: per block of 128 columns, row dots of C with aux, added to zeros
                    if g.epilogue != 128 or g.trans_a or g.trans_b or g.n % 128 or g.k % 16 or g.batch0 * g.batch1 != 1:
                        return UNSUPPORTED
                    prod = _mat(g.c + oc, g.m, g.n, g.ldc).astype(np.float64) * _mat(g.aux + oc, g.m, g.n, g.ldaux).astype(np.float64)
                    out = _vec(g.rowdot, (g.n // 128) * g.m).reshape(g.n // 128, g.m)
                    assert not np.isnan(out).any() and (out == 0).all(), 'NPM_EPI_ROWDOT: rowdot must be zero on entry'
                    out += (np.float64(g.rowdot_scale) * prod.reshape(g.m, g.n // 128, 128).sum(axis=2).T).astype(np.float32)
                sums[z1] += _mat(g.c + oc, g.m, g.n, g.ldc).astype(np.float64).sum(axis=0)
        if g.colsum:
            _vec(g.colsum, g.batch1 * g.n)[:] = sums.ravel()
        if g.bsum:
            assert not g.trans_b and g.batch0 == 1 and g.batch1 == 1
            _vec(g.bsum, g.n)[:] = _mat(g.b, g.k, g.n, g.ldb).astype(np.float64).sum(axis=0)
        if g.asum:
            assert g.trans_a and g.batch0 == 1 and g.batch1 == 1 and not g.bsum
            _vec(g.asum, g.m)[:] = _mat(g.a, g.k, g.m, g.lda).astype(np.float64).sum(axis=0)
        return 0

    # ---- elementwise ------------------------------------------------------------------------
    def npm_relu_fwd(self, x, y, n):
        _vec(y, n)[:] = np.maximum(_vec(x, n), 0)
        return 0

    def npm_relu_bwd(self, x, dy, dx, n):
        _vec(dx, n)[:] = np.where(_vec(x, n) >= 0, _vec(dy, n), 0)
        return 0

    def npm_add(self, a, b, out, n):
        self.calls.append('npm_add')
        _vec(out, n)[:] = _vec(a, n) + _vec(b, n)
        return 0

    def npm_add3(self, a, b, c, out, n):
        _vec(out, n)[:] = _vec(a, n) + _vec(b, n) + _vec(c, n)
        return 0

    def npm_axpy(self, y, x, alpha, n):
        self.calls.append('npm_axpy')
        _vec(y, n)[:] = _vec(y, n) + np.float32(alpha) * _vec(x, n)
        return 0

    def npm_scale(self, x, y, alpha, n):
        _vec(y, n)[:] = np.float32(alpha) * _vec(x, n)
        return 0

    def npm_colsum(self, x, out, rows, cols, ld):
        _vec(out, cols)[:] = _mat(x, rows, cols, ld).astype(np.float64).sum(axis=0)
        return 0

    def npm_relu_bwd_colsum(self, x, dy, dx, colsum, rows, cols):
        n = rows * cols
        g = np.where(_vec(x, n) >= 0, _vec(dy, n), 0)
        _vec(dx, n)[:] = g
        _vec(colsum, cols)[:] = g.reshape(rows, cols).astype(np.float64).sum(axis=0)
        return 0

    # ---- row kernels ---------------------------------------------------------------------------
    def npm_attn_rowdot(self, a, b, out, batch, seq, heads, dim):
        n = int(batch * seq * heads * dim)
        prod = (_vec(a, n).astype(np.float64) * _vec(b, n)).reshape(batch, seq, heads, dim).sum(axis=-1)
        _vec(out, batch * seq * heads)[:] = prod.transpose(0, 2, 1).ravel()
        return 0

    def npm_softmax_fwd(self, x, y, rows, n, scale):
        _mat(y, rows, n, n)[:] = O.softmax_fwd(np.float64(scale) * _mat(x, rows, n, n).astype(np.float64))
        return 0

    def npm_softmax_bwd(self, y, dy, dx, rows, n, scale):
        _mat(dx, rows, n, n)[:] = scale * O.softmax_bwd(_mat(y, rows, n, n), _mat(dy, rows, n, n))
        return 0

    def npm_layernorm_fwd(self, x, gamma, beta, eps, rows, d, z, mean, rstd):
        xv = _mat(x, rows, d, d).astype(np.float64)
        out, (mu, var, _) = O.layernorm_fwd(xv, _vec(gamma, d).astype(np.float64), _vec(beta, d).astype(np.float64), eps)
        _mat(z, rows, d, d)[:] = out
        _vec(mean, rows)[:] = mu[:, 0]
        _vec(rstd, rows)[:] = 1.0 / np.sqrt(var[:, 0] + eps)
        return 0

    def npm_layernorm_bwd(self, dz, x, mean, rstd, gamma, residual, rows, d, dx, dgamma, dbeta):
        xv = _mat(x, rows, d, d).astype(np.float64)
        mu = _vec(mean, rows).astype(np.float64)[:, None]
        rs = _vec(rstd, rows).astype(np.float64)[:, None]
        yhat = (xv - mu) * rs
        dzv = _mat(dz, rows, d, d).astype(np.float64)
        g = dzv * _vec(gamma, d).astype(np.float64)
        out = rs * (g - g.mean(axis=1, keepdims=True) - yhat * (g * yhat).mean(axis=1, keepdims=True))
        if _addr(residual):
            out = out + _mat(residual, rows, d, d)
        dg, db = (dzv * yhat).sum(axis=0), dzv.sum(axis=0)
        _mat(dx, rows, d, d)[:] = out
        _vec(dgamma, d)[:] = dg
        _vec(dbeta, d)[:] = db
        return 0

    def _dropped(self, x, mask, keep, rows, d):
        mk = np.ctypeslib.as_array((C.c_ubyte * int(rows * d)).from_address(_addr(mask))).reshape(rows, d) != 0
        return mk, np.where(mk, _mat(x, rows, d, d) / np.float32(keep), np.float32(0)).astype(np.float32)

    def npm_layernorm_dropout_fwd(self, x, mask, keep, gamma, beta, eps, rows, d, z, mean, rstd):
        """include/npm_hip.h: npm_mask_scale, then npm_layernorm_fwd, without the tensor in between."""
        self.calls.append('npm_layernorm_dropout_fwd')
        assert d % 4 == 0 and d <= 4096 and _addr(mask) % 4 == 0
        _, xd = self._dropped(x, mask, keep, rows, d)
        return self.npm_layernorm_fwd(xd.ctypes.data, gamma, beta, eps, rows, d, z, mean, rstd)

    def npm_layernorm_dropout_bwd(self, dz, x, mask, keep, mean, rstd, gamma, residual, rows, d, dx, dgamma, dbeta):
        self.calls.append('npm_layernorm_dropout_bwd')
        assert d % 4 == 0 and d <= 4096 and _addr(mask) % 4 == 0
        mk, xd = self._dropped(x, mask, keep, rows, d)
        inner = np.empty([rows, d], dtype=np.float32)
        rc = self.npm_layernorm_bwd(dz, xd.ctypes.data, mean, rstd, gamma, 0, rows, d, inner.ctypes.data, dgamma, dbeta)
        out = np.where(mk, inner / np.float32(keep), np.float32(0))
        if _addr(residual):
            out = out + _mat(residual, rows, d, d)
        _mat(dx, rows, d, d)[:] = out
        return rc

    def npm_rmsnorm_fwd(self, x, gamma, eps, rows, d, z, rstd):
        self.calls.append('npm_rmsnorm_fwd')
        rows, d = int(rows), int(d)
        if rows < 0 or d < 1:
            return BAD
        if rows == 0:
            return 0
        if not all(_addr(p) for p in (x, gamma, z, rstd)):
            return BAD
        out, rs = LR.rmsnorm_fwd(_mat(x, rows, d, d), _vec(gamma, d), eps)
        _mat(z, rows, d, d)[:] = out
        _vec(rstd, rows)[:] = rs[:, 0]
        return 0

    def npm_rmsnorm_bwd(self, dz, x, rstd, gamma, residual, rows, d, dx, dgamma):
        self.calls.append('npm_rmsnorm_bwd')
        rows, d = int(rows), int(d)
        if rows < 0 or d < 1 or not _addr(dgamma):
            return BAD
        if rows == 0:
            _vec(dgamma, d)[:] = 0
            return 0
        if not all(_addr(p) for p in (dz, x, rstd, gamma, dx)):
            return BAD
        # from the saved rstd, as the kernel: xh = x rstd
        xv, rs = _mat(x, rows, d, d).astype(np.float64), _vec(rstd, rows).astype(np.float64)[:, None]
        dzv, gm = _mat(dz, rows, d, d).astype(np.float64), _vec(gamma, d).astype(np.float64)
        xh, g = xv * rs, dzv * gm
        out = rs * (g - xh * (g * xh).mean(axis=1, keepdims=True))
        if _addr(residual):
            out = out + _mat(residual, rows, d, d)
        _mat(dx, rows, d, d)[:] = out
        _vec(dgamma, d)[:] = (dzv * xh).sum(axis=0)
        return 0

    def npm_swiglu_fwd(self, pre, ld, rows, units, h, ldh):
        self.calls.append('npm_swiglu_fwd')
        ld, rows, units, ldh = int(ld), int(rows), int(units), int(ldh)
        if rows < 0 or units < 1 or ld < 2 * units or ldh < units:
            return BAD
        if rows == 0:
            return 0
        if not (_addr(pre) and _addr(h)):
            return BAD
        with np.errstate(over='ignore', invalid='ignore'):
            _mat(h, rows, units, ldh)[:] = LR.swiglu_fwd(_mat(pre, rows, 2 * units, ld))
        return 0

    def npm_swiglu_bwd(self, pre, ld, dh, lddh, rows, units, dpre, lddpre):
        self.calls.append('npm_swiglu_bwd')
        ld, lddh, rows, units, lddpre = int(ld), int(lddh), int(rows), int(units), int(lddpre)
        if rows < 0 or units < 1 or ld < 2 * units or lddh < units or lddpre < 2 * units:
            return BAD
        if rows == 0:
            return 0
        if not (_addr(pre) and _addr(dh) and _addr(dpre)):
            return BAD
        with np.errstate(over='ignore', invalid='ignore'):
            _mat(dpre, rows, 2 * units, lddpre)[:] = LR.swiglu_bwd(_mat(pre, rows, 2 * units, ld), _mat(dh, rows, units, lddh))
        return 0

    # ---- fused attention core ------------------------------------------------------------------------
    def npm_mha_mask_summary(self, mask, sb, sh, sq_stride, nb, nh, seq_q, seq_kv, out):
        """byte (qt, kb) of plane (b, h): bit w = some allowed position in queries 32 qt.. x keys 128 kb + 16 w.. (include/npm_hip.h)"""
        self.calls.append('npm_mha_mask_summary')
        nqt, nkb = (seq_q + 31) // 32, (seq_kv + 127) // 128
        extent = (nb - 1) * sb + (nh - 1) * sh + (seq_q - 1) * sq_stride + seq_kv
        raw = np.ctypeslib.as_array((C.c_ubyte * int(extent)).from_address(_addr(mask)))
        planes = np.lib.stride_tricks.as_strided(raw, shape=(nb, nh, seq_q, seq_kv), strides=(sb, sh, sq_stride, 1))
        padded = np.zeros((nb, nh, nqt * 32, nkb * 128), dtype=bool)
        padded[:, :, :seq_q, :seq_kv] = planes != 0
        inside = np.zeros_like(padded)
        inside[:, :, :seq_q, :seq_kv] = True
        split = lambda a: a.reshape(nb, nh, nqt, 32, nkb, 8, 16)
        any16 = split(padded).any(axis=(3, 6))                                          # [nb, nh, nqt, nkb, 8]
        any16[~(planes != 0).any(axis=3).all(axis=2)] = True     # a plane with a key-less query row is never skipped (npm_hip.h)
        all16 = split(padded | ~inside).all(axis=(3, 6)) & split(inside).any(axis=(3, 6))
        pack = lambda bits: (bits << np.arange(8)).sum(axis=-1).astype(np.uint8).reshape(-1)
        both = np.concatenate([pack(any16), pack(all16)])
        np.ctypeslib.as_array((C.c_ubyte * both.size).from_address(_addr(out)))[:] = both
        return 0

    def npm_mha_core_supported(self, head_dim):
        return int(head_dim in (16, 32, 64, 128))

    def _core_mask(self, c):
        if not c.mask:
            return None
        b, h, sq, skv = c.batch, c.heads, c.seq_q, c.seq_kv
        extent = (b - 1) * c.mask_stride_b + (h - 1) * c.mask_stride_h + (sq - 1) * c.mask_stride_q + skv
        raw = np.ctypeslib.as_array((C.c_ubyte * int(extent)).from_address(_addr(c.mask)))
        return np.lib.stride_tricks.as_strided(raw, shape=(b, h, sq, skv),
                                               strides=(c.mask_stride_b, c.mask_stride_h, c.mask_stride_q, 1)) != 0

    def npm_mha_core_fwd(self, cref):
        c = _deref(cref)
        self.calls.append('npm_mha_core_fwd')
        if c.head_dim not in (16, 32, 64, 128):
            return UNSUPPORTED
        b, h, sq, skv, d = c.batch, c.heads, c.seq_q, c.seq_kv, c.head_dim
        q, k, v = (_heads(ptr, pitch, b, s, h, d).astype(np.float64)
                   for ptr, pitch, s in ((c.q, c.q_pitch, sq), (c.k, c.k_pitch, skv), (c.v, c.v_pitch, skv)))
        mask = self._core_mask(c)
        with np.errstate(invalid='ignore'):
            ctx, lse, _ = O.attention_core_fwd(q, k, v, float(c.scale), mask)
        _heads(c.ctx, c.ctx_pitch, b, sq, h, d)[:] = ctx
        _vec(c.lse, b * h * sq)[:] = lse.ravel()
        if c.scores:
            raw = np.einsum('bqhd,bkhd->bhqk', q, k)
            _vec(c.scores, b * h * sq * skv)[:] = (raw if mask is None else np.where(mask, raw, -np.inf)).ravel()
        return 0

    def npm_mha_core_bwd(self, cref):
        c = _deref(cref)
        self.calls.append('npm_mha_core_bwd')
        b, h, sq, skv, d = c.batch, c.heads, c.seq_q, c.seq_kv, c.head_dim
        q, k, v = (_heads(ptr, pitch, b, s, h, d).astype(np.float64)
                   for ptr, pitch, s in ((c.q, c.q_pitch, sq), (c.k, c.k_pitch, skv), (c.v, c.v_pitch, skv)))
        dctx = _heads(c.dctx, c.dctx_pitch, b, sq, h, d).astype(np.float64)
        lse = _vec(c.lse, b * h * sq).astype(np.float64).reshape(b, h, sq)
        scaled = float(c.scale) * np.einsum('bqhd,bkhd->bhqk', q, k)
        mask = self._core_mask(c)
        if mask is not None:
            scaled = np.where(mask, scaled, -np.inf)
        probs = np.exp(scaled - lse[..., None])             # from the saved log-sum-exp, as the kernel does
        if c.neg_delta:                                     # the caller's row terms: what the kernel would have computed itself
            ctx = _heads(c.ctx, c.ctx_pitch, b, sq, h, d).astype(np.float64)
            want = -float(c.scale) * np.einsum('bqhd,bqhd->bhq', dctx, ctx)
            extent = (b - 1) * c.neg_delta_stride_b + (h - 1) * c.neg_delta_stride_h + sq
            got = np.lib.stride_tricks.as_strided(_vec(c.neg_delta, extent), shape=(b, h, sq),
                                                  strides=(4 * c.neg_delta_stride_b, 4 * c.neg_delta_stride_h, 4))
            np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-5 * (np.abs(want).max() + 1e-30), err_msg='neg_delta')
        dq, dk, dv = O.attention_core_bwd(q, k, v, probs, dctx, float(c.scale))
        _heads(c.dq, c.dq_pitch, b, sq, h, d)[:] = dq
        _heads(c.dk, c.dk_pitch, b, skv, h, d)[:] = dk
        _heads(c.dv, c.dv_pitch, b, skv, h, d)[:] = dv
        return 0

    @staticmethod
    def _widened(c, kv_heads):
        """K and V expanded to one head per query head: query head h reads K / V head h % kv_heads."""
        return [np.ascontiguousarray(_heads(ptr, pitch, c.batch, c.seq_kv, kv_heads, c.head_dim)[:, :, np.arange(c.heads) % kv_heads])
                for ptr, pitch in ((c.k, c.k_pitch), (c.v, c.v_pitch))]

    def npm_mha_core_fwd_grouped(self, cref, kv_heads):
        """The ungrouped restatement on expanded K / V."""
        c = _deref(cref)
        self.calls.append('npm_mha_core_fwd_grouped')
        wide = self._widened(c, kv_heads)
        saved = (c.k, c.k_pitch, c.v, c.v_pitch)
        c.k, c.k_pitch, c.v, c.v_pitch = wide[0].ctypes.data, c.heads * c.head_dim, wide[1].ctypes.data, c.heads * c.head_dim
        try:
            return self.npm_mha_core_fwd(cref)
        finally:
            c.k, c.k_pitch, c.v, c.v_pitch = saved

    def npm_mha_core_bwd_grouped(self, cref, kv_heads):
        """The ungrouped restatement on expanded K / V; dK / dV of a K / V head are the sums over its query heads."""
        c = _deref(cref)
        b, h, skv, d = c.batch, c.heads, c.seq_kv, c.head_dim
        wide = self._widened(c, kv_heads)
        grads = [np.zeros([b, skv, h, d], dtype=np.float32) for _ in range(2)]
        saved = (c.k, c.k_pitch, c.v, c.v_pitch, c.dk, c.dk_pitch, c.dv, c.dv_pitch)
        c.k, c.k_pitch, c.v, c.v_pitch = wide[0].ctypes.data, h * d, wide[1].ctypes.data, h * d
        c.dk, c.dk_pitch, c.dv, c.dv_pitch = grads[0].ctypes.data, h * d, grads[1].ctypes.data, h * d
        try:
            rc = self.npm_mha_core_bwd(cref)
        finally:
            c.k, c.k_pitch, c.v, c.v_pitch, c.dk, c.dk_pitch, c.dv, c.dv_pitch = saved
        for grad, ptr, pitch in ((grads[0], c.dk, c.dk_pitch), (grads[1], c.dv, c.dv_pitch)):
            _heads(ptr, pitch, b, skv, kv_heads, d)[:] = grad.astype(np.float64).reshape(b, skv, h // kv_heads, kv_heads, d).sum(axis=2)
        return rc

    def npm_rope(self, x, pitch, batch, tokens, heads, head_dim, cos, sin, table_rows, at, at_lens, inverse):
        self.calls.append('npm_rope')
        self.ropes.append(dict(x=_addr(x), pitch=int(pitch), batch=batch, tokens=tokens, heads=heads, head_dim=head_dim,
                               table_rows=table_rows, at=at, at_lens=_addr(at_lens), inverse=int(inverse)))
        return self._rope(x, pitch, batch, tokens, heads, head_dim, cos, sin, table_rows, at, at_lens, inverse)

    def _rope(self, x, pitch, batch, tokens, heads, head_dim, cos, sin, table_rows, at, at_lens, inverse):
        """tests/rope_reference.py ``rotate``, the bitwise model of the kernel; rows outside the table are left untouched.  The
        caller records the call."""
        if not (_addr(x) and _addr(cos) and _addr(sin)):
            return BAD
        if min(batch, tokens, heads, table_rows) < 1 or head_dim < 2 or head_dim % 2 or pitch < heads * head_dim:
            return BAD
        if not _addr(at_lens) and (at < 0 or at + tokens > table_rows):
            return BAD
        half = head_dim // 2
        c, s = (_vec(t, table_rows * half).reshape(table_rows, half) for t in (cos, sin))
        rows = _heads(x, pitch, batch, tokens, heads, head_dim)
        start = _ints(at_lens, batch) if _addr(at_lens) else np.full(batch, at, dtype=np.int64)
        positions = start[:, None] + np.arange(tokens)[None, :]
        inside = (positions >= 0) & (positions < table_rows)
        rotated = RR.rotate(np.ascontiguousarray(rows), np.where(inside, positions, 0), c, s, inverse=bool(inverse))
        rows[inside] = rotated[inside]
        return 0

    # ---- conv -----------------------------------------------------------------------------------
    def npm_conv2d_fwd(self, cref):
        c = _deref(cref)
        x = _vec(c.x, c.n * c.h * c.w * c.c_in).reshape(c.n, c.h, c.w, c.c_in)
        f = _vec(c.filt, c.ksize * c.ksize * c.c_in * c.c_out).reshape(c.ksize, c.ksize, c.c_in, c.c_out)
        v = O.conv2d_fwd(x, f)
        if c.bias:
            v = v + _vec(c.bias, c.c_out)
        if c.relu:
            if c.pre:
                _vec(c.pre, v.size)[:] = v.ravel()
            v = np.maximum(v, 0)
        _vec(c.y, v.size)[:] = v.ravel()
        return 0

    def npm_conv2d_bwd_x(self, dy, filt, dx, n, h, w, c0, c1, k):
        g = _vec(dy, n * h * w * c1).reshape(n, h, w, c1)
        f = _vec(filt, k * k * c0 * c1).reshape(k, k, c0, c1)
        _vec(dx, n * h * w * c0)[:] = O.conv2d_grad_x(g, f).ravel()
        return 0

    def npm_conv2d_bwd_w(self, dy, x, dw, n, h, w, c0, c1, k):
        g = _vec(dy, n * h * w * c1).reshape(n, h, w, c1)
        xv = _vec(x, n * h * w * c0).reshape(n, h, w, c0)
        _vec(dw, k * k * c0 * c1)[:] = O.conv2d_grad_w(g, xv, k).ravel()
        return 0

    def npm_conv2d_bwd_w_relu(self, dy, pre, x, g, dw, db, n, h, w, c0, c1, k):
        size = n * h * w * c1
        gv = np.where(_vec(pre, size) >= 0, _vec(dy, size), 0).astype(np.float32)
        _vec(g, size)[:] = gv
        _vec(db, c1)[:] = gv.reshape(-1, c1).sum(axis=0)
        return self.npm_conv2d_bwd_w(g, x, dw, n, h, w, c0, c1, k)

    # ---- around the path -------------------------------------------------------------------------
    def npm_adam_step(self, var, grad, m, v, n, lr, beta1, beta2, eps, step):
        """csrc/npm_optim.hip adam_kernel = reference optimizer.py:58-63: the two gradient products in float32, the rest in float64."""
        self.calls.append('npm_adam_step')
        n = int(n)
        if step < 1:
            return BAD
        if n == 0:
            return 0
        if not (_addr(var) and _addr(grad) and _addr(m) and _addr(v)):
            return BAD
        mm = np.ctypeslib.as_array((C.c_double * n).from_address(_addr(m)))
        vv = np.ctypeslib.as_array((C.c_double * n).from_address(_addr(v)))
        g = _vec(grad, n)                                   # float32: the two products below stay float32
        with np.errstate(all='ignore'):
            mm[:] = beta1 * mm + np.float32(1 - beta1) * g
            vv[:] = beta2 * vv + np.float32(1 - beta2) * (g * g)
            upd = lr * ((mm / (1 - beta1 ** step)) / np.sqrt(vv / (1 - beta2 ** step) + eps))
        w = _vec(var, n)
        w -= upd                                            # fp64 loop, one rounding (as NumPy's f32 -= f64)
        return 0

    def npm_sumsq_ranges(self, ranges, acc):
        self.calls.append('npm_sumsq_ranges')
        if ranges is None or not _addr(acc):
            return BAD
        table = _deref(ranges)
        if not 0 <= table.count <= SUMSQ_MAX_RANGES:
            return BAD
        parts = [(int(table.ptr[i] or 0), int(table.n[i])) for i in range(table.count)]
        if any(n > 0 and (not ptr or ptr % 4) for ptr, n in parts):
            return BAD
        self.sumsq_tables.append(parts)
        if not any(n for _, n in parts):
            return 0
        total = AR.exact_sumsq(*[_vec(ptr, n) for ptr, n in parts if n])       # the exact sum, rounded once
        out = _words(acc, 1, C.c_double)
        with np.errstate(all='ignore'):
            out[0] = out[0] + total
        return 0

    def npm_clip_finish(self, state, max_norm):
        self.calls.append('npm_clip_finish')
        if not _addr(state) or not max_norm > 0.0:
            return BAD
        s = _words(state, 4, C.c_double)
        s[1], s[2], s[3] = AR.clip_finish(s[0], max_norm)
        return 0

    def npm_adamw_step(self, var, grad, m, v, n, lr, beta1, beta2, eps, step, weight_decay, clip_state):
        """tests/adamw_reference.py ``adamw_model``; a clip state whose step is not to be taken leaves everything as it is."""
        self.calls.append('npm_adamw_step')
        n = int(n)
        if step < 1 or not weight_decay >= 0.0:
            return BAD
        if n == 0:
            return 0
        if not (_addr(var) and _addr(grad) and _addr(m) and _addr(v)):
            return BAD
        clip = None
        if _addr(clip_state):
            s = _words(clip_state, 4, C.c_double)
            clip = (float(s[2]), float(s[3]))
            if clip[1] == 0:
                return 0                        # nothing at all is written
        mm, vv = _words(m, n, C.c_double), _words(v, n, C.c_double)
        out = AR.adamw_model(_vec(var, n), _vec(grad, n), mm, vv, int(step), (lr, beta1, beta2, eps), weight_decay, clip)
        mm[:], vv[:] = out.m, out.v
        _vec(var, n)[:] = out.p
        return 0

    def npm_mse_fwd(self, y, t, n, out):
        if int(n) == 0 or not (_addr(y) and _addr(t)):
            return BAD
        d = _vec(y, n).astype(np.float64) - _vec(t, n)
        _deref(out).value = float((d * d).sum() / int(n))
        return 0

    def npm_mse_bwd(self, y, t, dy, n):
        if int(n) == 0:
            return 0
        _vec(dy, n)[:] = np.float32(2.0 / int(n)) * (_vec(y, n) - _vec(t, n))
        return 0

    def npm_xent_fwd(self, y, t, n, out):
        if int(n) == 0 or not (_addr(y) and _addr(t)):
            return BAD
        with np.errstate(all='ignore'):
            _deref(out).value = float(-(_vec(t, n).astype(np.float64) * np.log(_vec(y, n).astype(np.float64))).sum())
        return 0

    def npm_xent_bwd(self, y, t, dy, n):
        if int(n) == 0:
            return 0
        with np.errstate(all='ignore'):
            _vec(dy, n)[:] = -_vec(t, n) / _vec(y, n)
        return 0

    def npm_softmax_xent_rows(self, logits, ld, targets, rows, vocab, smoothing, grad_scale, dlogits, ldd, row_loss, row_lse, loss_sum):
        """tests/xent_reference.py ``reference`` over the rows that have a target."""
        self.calls.append('npm_softmax_xent_rows')
        rows, vocab, ld, ldd = int(rows), int(vocab), int(ld), int(ldd)
        z_at, d_at = _addr(logits), _addr(dlogits)
        if loss_sum is None or not 0 <= rows < 2 ** 31 or not 1 <= vocab <= 2 ** 30 or ld < vocab or not 0.0 <= smoothing < 1.0:
            return BAD
        if d_at and ldd < vocab:
            return BAD
        if rows == 0:
            self.last_xent = b'xent_none rows=0'
            _deref(loss_sum).value = 0.0
            return 0
        if not z_at or not _addr(targets) or not _addr(row_loss):
            return BAD
        if d_at == z_at and d_at:
            if ldd != ld:
                return BAD
        elif d_at:
            z_end, d_end = z_at + 4 * ((rows - 1) * ld + vocab), d_at + 4 * ((rows - 1) * ldd + vocab)
            if not (z_end <= d_at or d_end <= z_at):
                return BAD
        t = _ints(targets, rows)
        z = _mat(logits, rows, vocab, ld)
        # an ignored row is not read: it may hold anything
        seen = np.where((t >= 0)[:, None], z, 0.0).astype(np.float64)
        ref = xent_reference.reference(seen, t, smoothing, grad_scale, need_grad=bool(d_at))
        with np.errstate(over='ignore'):
            if d_at:
                _mat(dlogits, rows, vocab, ldd)[:] = ref.grad.astype(np.float32)
            _vec(row_loss, rows)[:] = ref.row_loss.astype(np.float32)
            if _addr(row_lse):
                _vec(row_lse, rows)[:] = ref.lse.astype(np.float32)
        _deref(loss_sum).value = float(_vec(row_loss, rows).astype(np.float64).sum())
        vec = z_at % 16 == 0 and ld % 4 == 0 and (not d_at or (d_at % 16 == 0 and ldd % 4 == 0))
        self.last_xent = ('%s V=%d grad=%d inplace=%d vec=%d nt=%d' % (xent_cases.instance_of(vocab), vocab, bool(d_at), d_at == z_at,
                                                                       vec, 4 * rows * vocab >= 32 << 20)).encode()
        return 0

    def npm_last_xent_kernel(self):
        return self.last_xent

    def npm_mask_scale(self, x, mask, y, n, keep):
        self.calls.append('npm_mask_scale')
        if int(n) == 0:
            return 0
        if not (_addr(x) and _addr(mask) and _addr(y) and keep > 0):
            return BAD
        mk = np.ctypeslib.as_array((C.c_ubyte * int(n)).from_address(_addr(mask)))
        _vec(y, n)[:] = np.where(mk != 0, _vec(x, n) / np.float32(keep), 0)
        return 0

    def npm_dropout_philox(self, x, y, mask, n, keep, seed, offset):
        self.calls.append('npm_dropout_philox')
        if int(n) == 0:
            return 0
        if not _addr(mask) or bool(_addr(x)) != bool(_addr(y)) or not 0.0 < keep <= 1.0:
            return BAD
        keep_mask = O.dropout_philox_mask(int(n), float(keep), int(seed), int(offset))
        np.ctypeslib.as_array((C.c_ubyte * int(n)).from_address(_addr(mask)))[:] = keep_mask
        if _addr(y):                               # x = y = NULL: the mask only
            _vec(y, n)[:] = np.where(keep_mask, _vec(x, n) / np.float32(keep), 0)
        return 0

    def npm_last_attn_kernel(self):
        last = [c for c in self.calls if c.startswith('npm_mha_core_')]
        return (('hostsim ' + last[-1]) if last else '').encode()
