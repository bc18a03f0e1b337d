"""Float64 numpy model of vaeq_dp_epilogue_llr and vaeq_awgn_llr: the per-bit a-posteriori LLRs of the DP and AWGN soft demappers, written from
the definition (the reference has no such output).  Roll, polarisation exchange and kept window are tests/_ref_epilogue.py's (DP) and
tests/_ref_awgn_info.py's (AWGN); the posteriors are tests/_ref_info.py's and tests/_ref_awgn_info.py's.

Level i of an axis carries the label g(i) = i ^ (i >> 1), b = log2 n bits, bit b-1 the top one.  For one symbol and one received axis c
    lam[c][k] = ln 2 (L[c][k][0] - L[c][k][1])      nats, positive = bit 0, a-posteriori
L[c][k][s] = log2 of the posterior mass of the levels whose label bit k is s: q-mode log2 max(sum, FLT_MIN) of the stored q, y-mode an exact
log-sum-exp of the demapper's exponent.  Hypothesis h = 4 flip + rot, rot in (0, pi, pi/2, 3 pi/2):
    I' = axis 0 | axis 0 reversed | axis 1 reversed | axis 1,     Q' = axis 1 | axis 1 reversed | axis 0 | axis 0 reversed,
the flip reversing Q' once more; "reversed" negates the top-bit plane of that axis.  Output plane a b + k = bit k of TX axis a at the TX symbol
index; everything the window does not keep is an erasure, 0.

Test infrastructure only.  Every function returns (planes[..., 2b, N] float64, kept mask[..., N] bool).  llr_y32 is y-mode in numpy float32 in
the kernels' operation order, the counterpart of _ref_info.y_mode_float32_deviation.
"""
import numpy as np

import _ref_awgn_info as A
import _ref_epilogue as E
import _ref_info as I

LN2 = float(np.log(2.0))
FLT_MIN = I.FLT_MIN
# the largest |float32 emulation - float64 model| / max(1, |model|) of y-mode over the kept entries of every launch of _ref_info.LAUNCHES (DP:
# 3.57e-7, with |lam| up to 400 nats) and of _ref_awgn_info.LAUNCHES (AWGN: 4.38e-6, with |lam| up to 600 nats -- there the float32 sum of |y_c|
# over the row moves the scale of every sample, and a relative error of 1e-7 in yhat is one of a few 1e-6 in (yhat - a_i)^2 differences),
# computed and asserted on the CPU by tests/test_ref_llr_host.py, rounded up.  The GPU tests hold y-mode to four times these.
Y_LLR_DEV = 3.6e-7
Y_LLR_DEV_AWGN = 4.4e-6


def nbits(n):
    return int(round(np.log2(n)))


def label_bits(tx, n):
    """tx[..., 2, N] -> int64[..., 2b, N]: plane a b + k = bit k of the Gray label of axis a's level (info_tx_level's quantisation)."""
    b = nbits(n)
    g = I.gray(A.tx_levels(np.asarray(tx, np.float64), n))
    bits = (g[..., :, None, :] >> np.arange(b)[:, None]) & 1
    return bits.reshape(g.shape[:-2] + (2 * b, g.shape[-1]))


def set_llr_q(q, n):
    """q[..., n, K] posteriors of one axis -> lam[..., b, K]."""
    g = I.gray(np.arange(n))
    out = []
    for k in range(nbits(n)):
        s = [np.log2(np.maximum(np.where((((g >> k) & 1) == v)[:, None], q, 0.0).sum(-2), FLT_MIN)) for v in (0, 1)]
        out.append(LN2 * (s[0] - s[1]))
    return np.stack(out, -2)


def set_llr_z(z, n, f=np.float64):
    """z[..., n, K] log2 of unnormalised posteriors of one axis -> lam[..., b, K]; every set a log-sum-exp around its own maximum, in format f
    (float32: each operation rounded, the kernels' order)."""
    g = I.gray(np.arange(n))
    z = np.asarray(z, f)
    out = []
    for k in range(nbits(n)):
        s = []
        for v in (0, 1):
            w = z[..., np.flatnonzero(((g >> k) & 1) == v), :]
            mx = w.max(-2)
            sm = np.zeros_like(mx)
            for i in range(w.shape[-2]):                                       # ascending i
                sm = (sm + np.exp2((w[..., i, :] - mx).astype(f)).astype(f)).astype(f)
            s.append((mx + np.log2(sm).astype(f)).astype(f))
        out.append((f(LN2) * (s[0] - s[1]).astype(f)).astype(f))
    return np.stack(out, -2)


def transform(lam, h, n):
    """lam[2 received axes][b][K] -> planes[2b][K] of the TX axes under hypothesis h = 4 flip + rot."""
    b = nbits(n)
    rot, flip = h & 3, (h >> 2) & 1
    (cI, rI), (cQ, rQ) = [((0, False), (1, False)), ((0, True), (1, True)), ((1, True), (0, False)), ((1, False), (0, True))][rot]
    rQ = rQ != bool(flip)
    out = np.concatenate([lam[cI], lam[cQ]], 0).copy()
    if rI:
        out[b - 1] = -out[b - 1]
    if rQ:
        out[2 * b - 1] = -out[2 * b - 1]
    return out


def retransform(planes, h, n):
    """The planes[..., 2b, N] under hypothesis 0 -> the planes under hypothesis h (planes exchanged, top-bit planes negated)."""
    lam = np.moveaxis(planes, -2, 0)
    b = nbits(n)
    out = transform(np.stack([lam[:b], lam[b:]]), h, n)
    return np.moveaxis(out, 0, -2)


# ------------------------------------------------------------------ DP
def _dp_place(lam_rx, N, n, shift, r, batch_len, hyp):
    """lam_rx[2 received rows][2 axes][b][N] -> (planes[2][2b][N] in TX order, mask[2][N])."""
    b = nbits(n)
    al = E.align(lam_rx.reshape(2, 2 * b, N), shift, r).reshape(2, 2, b, N)
    idx = E.kept_indices(N, shift, batch_len)
    mask = np.zeros((2, N), bool)
    planes = np.zeros((2, 2 * b, N), lam_rx.dtype)
    for p in range(2):
        m = idx + int(shift[p])
        ok = idx[(m >= 0) & (m < N)]
        mask[p, ok] = True
        planes[p][:, ok] = transform(al[p][:, :, ok], int(hyp[p]) & 7, n)
    return planes, mask


def dp_llr_q(q, n, shift, r, hyp, batch_len=None):
    """q[2][2n][N] as stored (float32 values, evaluated in float64), shift[2], r, hyp[2]."""
    N = q.shape[-1]
    lam = set_llr_q(np.asarray(q, np.float64).reshape(2, 2, n, N), n)
    return _dp_place(lam, N, n, shift, r, batch_len, hyp)


def _dp_z(y, amp, nu_sc, var, f):
    """The soft demapper's exponent in log2 per received row: float64 exact, float32 in info_demap_log2's order (a fused multiply-add where the
    compiler contracts is within the rounding this emulation measures)."""
    a = np.asarray(amp, f)
    y = np.asarray(y, f)
    z = np.empty((2, 2, len(a), y.shape[-1]), f)
    for sp in range(2):
        i2v = f(0.5) / f(np.asarray(var, f)[sp])
        for i in range(len(a)):
            dd = (y[sp] - a[i]).astype(f)
            z[sp, :, i] = (-(((dd * dd).astype(f) * i2v).astype(f) + f(f(nu_sc) * f(a[i] * a[i]))).astype(f) * f(1.4426950408889634)).astype(f)
    return z


def dp_llr_y(y, n, amp, nu_sc, var, shift, r, hyp, batch_len=None, f=np.float64):
    """y[2][2][N] float32; the posteriors are the soft demapper's with the RECEIVED row's var."""
    N = y.shape[-1]
    lam = set_llr_z(_dp_z(y, amp, nu_sc, var, f), n, f)
    return _dp_place(lam, N, n, shift, r, batch_len, hyp)


def dp_llr_y32(y, n, amp, nu_sc, var, shift, r, hyp, batch_len=None):
    return dp_llr_y(y, n, amp, nu_sc, var, shift, r, hyp, batch_len, np.float32)


# ------------------------------------------------------------------ AWGN
def _awgn_place(lam, N, n, shift, hyp):
    """lam[2 axes][b][N] (None: no normalisation) -> (planes[2b][N], mask[N])."""
    b = nbits(n)
    ri, ti = A.window(N, shift)
    mask = np.zeros(N, bool)
    planes = np.zeros((2 * b, N), np.float64 if lam is None else lam.dtype)
    if lam is not None and len(ti):
        mask[ti] = True
        planes[:, ti] = transform(lam[:, :, ri], int(hyp) & 3, n)
    return planes, mask


def awgn_llr_q(q, n, shift, hyp):
    """q[2n][N] as stored, shift, hyp."""
    N = q.shape[-1]
    return _awgn_place(set_llr_q(np.asarray(q, np.float64).reshape(2, n, N), n), N, n, shift, hyp)


def awgn_llr_y(y, n, amp, amp_mean, var, shift, hyp):
    """y[2][N] float32; yhat_c = y_c amp_mean / mean|y_c| over the whole row, z_i = -(yhat_c - a_i)^2 / var."""
    N = y.shape[-1]
    yh = A.normalised(y, amp_mean)
    if yh is None:
        return _awgn_place(None, N, n, shift, hyp)
    a = np.asarray(amp, np.float64)
    z = -(yh[:, None, :] - a[None, :, None]) ** 2 / float(var) * np.log2(np.e)
    return _awgn_place(set_llr_z(z, n), N, n, shift, hyp)


def awgn_llr_y32(y, n, amp, amp_mean, var, shift, hyp):
    """awgn_llr_y in numpy float32 in the kernel's operation order (the sums of |y_c| per thread at stride 256 and then over the threads, one scale
    per component, z = -(d d) (log2 e / var)), as _ref_awgn_info.y_mode_float32."""
    f = np.float32
    N = y.shape[-1]
    if len(A.window(N, shift)[0]) == 0:
        return _awgn_place(None, N, n, shift, hyp)
    sa = [np.array([np.abs(y[c, t::256]).sum(dtype=f) for t in range(min(256, N))], f).sum(dtype=f) for c in range(2)]
    if sa[0] == 0 or sa[1] == 0:
        return _awgn_place(None, N, n, shift, hyp)
    a = np.asarray(amp, f)
    ivl = f(f(1.4426950408889634) / f(var))
    z = np.empty((2, n, N), f)
    for c in range(2):
        yv = (y[c] * (f(amp_mean) / f(sa[c] / f(N)))).astype(f)
        for i in range(n):
            dd = (yv - a[i]).astype(f)
            z[c, i] = (-(dd * dd).astype(f) * ivl).astype(f)
    return _awgn_place(set_llr_z(z, n, f), N, n, shift, hyp)


# ------------------------------------------------------------------ what the tests compute from LLRs
def gmi_from_llr(planes, bits, mask, H):
    """2 H - mean over the kept symbols of sum_planes log2(1 + exp(-(1 - 2 bit) lam)); planes[2b][N], bits[2b][N], mask[N] -> float (NaN: nothing kept)."""
    if not mask.any():
        return float("nan")
    x = -(1.0 - 2.0 * bits[:, mask]) * np.asarray(planes, np.float64)[:, mask]
    return 2 * H - float((np.logaddexp(0.0, x) / LN2).sum(0).mean())


def sign_errors(planes, bits, mask):
    """Kept plane entries whose sign says the other bit (lam > 0 = bit 0; a zero LLR counts as bit 0)."""
    return int(((np.asarray(planes)[:, mask] < 0).astype(np.int64) != bits[:, mask]).sum())


def rel_dev(got, want, mask):
    """Largest |got - want| / max(1, |want|) over the kept entries (0 when nothing is kept)."""
    m = np.broadcast_to(mask[..., None, :], want.shape)
    if not m.any():
        return 0.0
    g, w = np.asarray(got, np.float64)[m], np.asarray(want, np.float64)[m]
    return float((np.abs(g - w) / np.maximum(1.0, np.abs(w))).max())
