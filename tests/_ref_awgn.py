"""Float64 numpy restatement of the AWGN baselines, written from the math of AWGN_channel/func_CMA_MQAM_shaping.py -- SER_CMA (:63-94),
find_shift_symb (:127-140), CMA (:142-168), CPE (:170-198), the evaluated epoch (:225-232) -- and AWGN_channel/DFE_MQAM_shaping.py --
SER_func (:107-135), find_shift_symb (:139-152), dfe (:200-222), nearest_neighbor (:224-234), compl_conv (:236-241), the LMMSE and DFE
evaluation (:276-293).

Test infrastructure only: nothing in the package imports it.  Layouts are the kernels': rx[2][N] = [re/im][sample], h[2][M], out[2][K],
K = N // sps, data[2][K] (the fp16 TX symbols), decisions as indices iI * n + iQ.

What it keeps from the reference, on purpose:
- CMA zero-pads the UNSCALED frame by mh = M // 2; symbol j (padded centre i = mh + sps j, :155) is stored at k = i // sps - mh (:157), which
  is negative for the first mh - mh // sps symbols and then wraps to the end of out / e like a tensor index; a later symbol at the same index
  overwrites it.  The taps move after every symbol (:164-166), not at all with eval=False.
- CPE (:189) takes atan2(im, -re) / 4 of the zero-padded 501-tap mean of the 4th power and does NOT unwrap: the correction jumps by pi/2
  where the averaged phasor crosses the cut of atan2.
- find_shift_symb compares the I-rail peak with 0.02 * rx.shape[-1] (:133), falls back to the Q rail of tx only when that rail's peak is at
  least the I peak (:137), and otherwise keeps the I-rail argmax (:140).
- SER_CMA / SER_func rescale by mean|tx| / mean|rx| over ALL samples of the rx slice (:73, :117), decide on its first tx.shape[1] samples
  (:74, :118), turn tx into level indices by round(scale * tx + scale) (:72, :116) and take the minimum over four relabelings (:76-91).
- The evaluation slices are written with negative ends (:231, DFE :282, :293): data[:, c + 11 : -11 - shift - c].  When 11 + shift + c == 0
  that end is -0 = 0 and the slice is EMPTY in the reference, while the kernels read the full slice (shift = -11 at N_shift = 23 in the CMA
  script's geometry).  The model raises ValueError there; no fixture lands on it.
- nearest_neighbor is restated as per-axis slicing (first index on ties), which is what the kernels do; it differs from the argmin over all
  n^2 complex distances only where two distances round equal.
"""
from bisect import bisect_left

import numpy as np

M_MA = 501                                                             # :172


# ------------------------------------------------------------------------------------------------------------------ helpers
def qam_levels(n_lev):
    """The per-axis levels of unit-power square QAM as float32 (the kernels' amp table)."""
    return (np.arange(-(n_lev - 1), n_lev, 2) / np.sqrt(2 * (n_lev ** 2 - 1) / 3)).astype(np.float32)


def _mids(levels):
    lev = np.asarray(levels, np.float64)
    return (lev[:-1] + lev[1:]) / 2


def slice_axis(v, levels):
    """Nearest level per coordinate, first index on ties (torch.argmin) -> (indices, distance to the nearest decision boundary)."""
    mids = _mids(levels)
    v = np.asarray(v, np.float64)
    idx = np.searchsorted(mids, v, side="left")                        # the number of boundaries strictly below v: a tie keeps the lower level
    return idx, np.min(np.abs(v[..., None] - mids), axis=-1)


# ------------------------------------------------------------------------------------------------------------------ CMA (:142-168)
def cma_symbol_indices(N, sps, M):
    """Output index of every symbol after the wrap (:157): symbol j -> (mh + sps j) // sps - mh, negative ones + K."""
    if N % sps:
        raise ValueError(f"{N} samples are no whole number of symbols at {sps} samples per symbol")
    mh, K = M // 2, N // sps
    kraw = (mh + sps * np.arange(K)) // sps - mh
    if len(kraw) and (kraw[0] < -K or kraw[-1] >= K):
        raise IndexError(f"symbol index out of bounds for {K} outputs")
    return np.where(kraw < 0, kraw + K, kraw)


def awgn_cma(rx, h, lr, sps, update=True, Rc=1.0):
    """rx[2,N], h[2,M] (not modified) -> (out[2,K], h_final[2,M], e[K], loss = mean|e| in symbol order).  In complex notation
    out = sum_t y[t] h[t] (:159-160) and the increment of :165-166 is 2 lr e out conj(y[t])."""
    rx = np.asarray(rx, np.float64)
    hc = np.asarray(h, np.float64)[0] + 1j * np.asarray(h, np.float64)[1]
    M, N = hc.shape[0], rx.shape[1]
    mh, K = M // 2, N // sps
    y = np.zeros(N + 2 * mh, complex)
    y[mh:mh + N] = rx[0] + 1j * rx[1]                                  # :149-150
    kk = cma_symbol_indices(N, sps, M)                                 # one index per symbol, a permutation of 0 .. K-1
    W = np.lib.stride_tricks.sliding_window_view(y, M)[::sps][:K]      # [symbol][tap] (:156)
    if not update or lr == 0:
        oc = W @ hc
    else:
        oc = np.empty(K, complex)
        for j in range(K):
            o = W[j] @ hc
            oc[j] = o
            hc = hc + (2 * lr * (Rc - abs(o) ** 2) * o) * np.conj(W[j])
    es = Rc - np.abs(oc) ** 2                                          # :162
    out, e = np.empty((2, K)), np.empty(K)
    out[0, kk], out[1, kk], e[kk] = oc.real, oc.imag, es               # in symbol order: the last write to an index would win
    return out, np.stack([hc.real, hc.imag]), e, float(np.mean(np.abs(es)))


def cma_frame(seed, N, sps, M, n_lev=2, drift=0.0, noise=0.05):
    """A QAM frame at sps samples per symbol (triangular pulse), a little ISI, a carrier phase ramp of `drift` rad over the frame, noise; taps:
    a perturbed Dirac, so that every tap takes part from the first symbol on.  -> rx[2,N] f32, h0[2,M] f32."""
    rng = np.random.default_rng(seed)
    K = -(-N // sps)
    lev = qam_levels(n_lev).astype(np.float64)
    s = lev[rng.integers(0, n_lev, K)] + 1j * lev[rng.integers(0, n_lev, K)]
    up = np.zeros(K * sps, complex)
    up[::sps] = s
    pulse = np.convolve(np.ones(sps), np.ones(sps))[sps - 1:] / sps if sps > 1 else np.ones(1)
    x = np.convolve(up, pulse)[:N]
    x[1:] += (0.12 - 0.05j) * x[:-1]
    x = x * np.exp(1j * (0.2 + drift * np.arange(N) / N))
    x += noise * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    h0 = (0.01 * rng.standard_normal((2, M))).astype(np.float32)
    h0[0, M // 2] += 1
    return np.stack([x.real, x.imag]).astype(np.float32), h0


# ------------------------------------------------------------------------------------------------------------------ CPE (:170-198)
def cpe(y):
    """y[2,K] -> (corrected y[2,K], modulus[K] of the averaged 4th-power phasor, angular distance[K] of it to the cut of atan2)."""
    y = np.asarray(y, np.float64)
    a, b = y[0], y[1]
    a2, b2 = a * a, b * b
    p4 = (a2 * a2 - 6 * a2 * b2 + b2 * b2) + 1j * (4 * (a2 * a * b - a * b2 * b))      # :180
    half = M_MA // 2
    cs = np.concatenate([[0], np.cumsum(np.pad(p4, (half, half)))])
    ma = (cs[M_MA:] - cs[:-M_MA]) / M_MA                               # :184-187 (zero-padded mean)
    ang = np.arctan2(ma.imag, -ma.real)
    phi = ang / 4                                                      # :189
    c, s = np.cos(phi), np.sin(phi)
    return np.stack([a * c - b * s, b * c + a * s]), np.abs(ma), np.pi - np.abs(ang)


def cpe_flags(modulus, dist):
    """Symbols where one float32 rounding may turn the correction by pi/2: the averaged phasor within 1e-3 rad of the cut, or its modulus
    below 1e-3 of the frame median."""
    return (dist < 1e-3) | (modulus < 1e-3 * np.median(modulus))


# ------------------------------------------------------------------------------------------------------------------ the evaluation tail
def find_shift(track_I, tx, n_shift, length):
    """(:127-140) -> (shift, |corr| of the I rail [n_shift], |corr| of the Q rail [n_shift], branch in {"I", "Q", "I kept"})."""
    hsh = n_shift // 2
    nm = 1000 - hsh
    tI = np.asarray(track_I, np.float64)
    tx = np.asarray(tx, np.float64)
    mat = np.stack([tI[i:i + nm] for i in range(n_shift)], axis=1)     # :128-131
    cI, cQ = np.abs(tx[0, hsh:1000] @ mat), np.abs(tx[1, hsh:1000] @ mat)
    if cI.max() >= 0.02 * length:                                      # :133
        return int(np.argmax(cI)) - hsh, cI, cQ, "I"
    if cQ.max() >= cI.max():                                           # :137
        return int(np.argmax(cQ)) - hsh, cI, cQ, "Q"
    return int(np.argmax(cI)) - hsh, cI, cQ, "I kept"


def ser(track, tx, levels):
    """track[2,Lr], tx[2,L] (Lr >= L) -> (counts[4] of the 0 / pi / pi/4 / 3pi/4 relabelings, winner = first minimum, distance[2,L] of every
    decided coordinate to the nearest decision boundary, decisions[2,L])."""
    track, tx = np.asarray(track, np.float64), np.asarray(tx, np.float64)
    lev = np.asarray(levels, np.float64)
    L, top = tx.shape[1], len(lev) - 1
    sc = top / 2
    t = np.rint(sc * tx + sc).astype(np.int64)                         # :72
    scale = np.mean(np.hypot(tx[0], tx[1])) / np.mean(np.hypot(track[0], track[1]))      # :73, over all Lr samples
    d, dist = slice_axis(track[:, :L] * scale, lev)                    # :74-76
    cands = (d, top - d, np.stack([top - d[1], d[0]]), np.stack([d[1], top - d[0]]))      # :76, :80, :85, :90
    counts = np.array([int(np.any(t != c, axis=0).sum()) for c in cands])
    return counts, int(np.argmin(counts)), dist, d


def _eval_slices(n_track, n_data, shift, n_cut):
    """The reference's slices rx[:, c+11+shift : -11-c], data[:, c+11 : -11-shift-c] as (start, stop) pairs; raises where the data slice's
    negative end is -0."""
    end = -11 - shift - n_cut
    if end >= 0:
        raise ValueError(f"shift {shift} with N_cut {n_cut}: the reference's data slice [:{end}] is empty")
    return (n_cut + 11 + shift, n_track - 11 - n_cut), (n_cut + 11, n_data + end)


def validate(rx, h, data, levels, sps, n_shift):
    """The evaluated epoch (:227-232) -> dict(out, cpe, modulus, dist, shift, cI, cQ, branch, counts, winner, margin, L)."""
    out, _, _, _ = awgn_cma(rx, h, 0.0, sps, update=False)
    y, mod, dist = cpe(out)
    K = y.shape[1]
    shift, cI, cQ, branch = find_shift(y[0], data, n_shift, K)
    (r0, r1), (d0, d1) = _eval_slices(K, K, shift, 0)
    counts, winner, margin, _ = ser(y[:, r0:r1], np.asarray(data, np.float64)[:, d0:d1], levels)
    return dict(out=out, cpe=y, modulus=mod, dist=dist, shift=shift, cI=cI, cQ=cQ, branch=branch, counts=counts, winner=winner,
                margin=margin, L=d1 - d0)


def compl_conv(rx, taps):
    """(:236-241) rx complex [N], taps complex [K] -> out[i] = sum_t x[i + t - K//2] taps[K-1-t], N + 2 (K//2) - K + 1 outputs."""
    x, t = np.asarray(rx, np.complex128), np.asarray(taps, np.complex128)
    K, N = len(t), len(x)
    No = N + 2 * (K // 2) - K + 1
    return np.convolve(x, t)[K - 1 - K // 2:][:No]


def lmmse(rx, taps, data, levels, n_shift, n_cut):
    """(:276-282) rx[2,N] -> dict(out complex [No], dec[N] of out[1:], dec_margin[N], shift, cI, cQ, branch, counts, winner, margin, L, Lr)."""
    rx = np.asarray(rx, np.float64)
    N = rx.shape[1]
    n = len(levels)
    out = compl_conv(rx[0] + 1j * rx[1], taps)
    No = len(out)
    o = out[1:1 + N]                                                   # :278
    dI, mI = slice_axis(o.real, levels)
    dQ, mQ = slice_axis(o.imag, levels)
    shift, cI, cQ, branch = find_shift(out.real, data, n_shift, No)    # :281
    (r0, r1), (d0, d1) = _eval_slices(No, N, shift, n_cut)
    track = np.stack([out.real, out.imag])[:, r0:r1]
    counts, winner, margin, _ = ser(track, np.asarray(data, np.float64)[:, d0:d1], levels)
    return dict(out=out, dec=dI * n + dQ, dec_margin=np.minimum(mI, mQ), shift=shift, cI=cI, cQ=cQ, branch=branch, counts=counts,
                winner=winner, margin=margin, L=d1 - d0, Lr=r1 - r0)


def dfe(ff, fb, init, levels):
    """(:200-222) ff complex [N], fb complex [K2], init[N] indices -> (decisions[N], the smallest distance of any sliced value to a decision
    boundary over the whole run).  Per-axis slicing, first index on ties."""
    lev = [float(v) for v in np.asarray(levels, np.float64)]
    mids = [float(v) for v in _mids(levels)]
    n, K2, N = len(lev), len(fb), len(ff)
    f = [complex(v) for v in np.asarray(fb, np.complex128)]
    v = [complex(x) for x in np.asarray(ff, np.complex128)]
    out = [int(i) for i in np.asarray(init)[:K2]] + [0] * (N - K2)
    st = [complex(lev[i // n], lev[i % n]) for i in out[:K2]]          # :213-214
    st += [0j] * (N - K2)
    margin = np.inf
    for p in range(K2, N):
        y = v[p]
        for j in range(K2):
            y += f[j] * st[p - 1 - j]                                  # :217
        iI, iQ = bisect_left(mids, y.real), bisect_left(mids, y.imag)
        margin = min(margin, min(abs(y.real - m) for m in mids), min(abs(y.imag - m) for m in mids))
        out[p] = iI * n + iQ
        st[p] = complex(lev[iI], lev[iQ])
    return np.array(out, np.int64), float(margin)


def dfe_eval(dec, data, levels, n_shift, n_cut):
    """(:290-293) find_shift_symb and SER_func on the hard decisions -> dict(shift, cI, cQ, branch, counts, winner, margin, L)."""
    lev = np.asarray(levels, np.float64)
    n, N = len(lev), len(dec)
    track = np.stack([lev[np.asarray(dec) // n], lev[np.asarray(dec) % n]])
    shift, cI, cQ, branch = find_shift(track[0], data, n_shift, N)
    (r0, r1), (d0, d1) = _eval_slices(N, N, shift, n_cut)
    counts, winner, margin, _ = ser(track[:, r0:r1], np.asarray(data, np.float64)[:, d0:d1], levels)
    return dict(shift=shift, cI=cI, cQ=cQ, branch=branch, counts=counts, winner=winner, margin=margin, L=d1 - d0)


# ------------------------------------------------------------------------------------------------------------------ conditioned fixtures
def conditioned_eval_frame(seed, K, n_lev, rot, lag, n_err, extra=0, gain=1.0, pert=0.25, validator=None):
    """A track of K + extra samples that is the TX sequence under the rotation rot * pi/2 and the lag `lag` (track[m + lag] ~ tx[m]), scaled by
    `gain`, plus a perturbation drawn uniformly from +-pert level spacings per coordinate, and TX data [2,K] (fp16) in which n_err symbols
    of the evaluated slice were swapped for a neighbour: the number of symbol errors is n_err by construction.

    validator = (sps, M, side): also the rx[2, K sps] and h[2,M] from which the CMA validation kernel produces such a track: only every
    sps-th sample is non-zero, h is a centre spike times a complex constant (whose small phase the CPE takes out again) with side taps of size
    `side` level spacings on the two neighbouring symbols.
    -> dict(track complex [K + extra], data f16 [2,K], levels f32, injected (indices), rx, h)."""
    rng = np.random.default_rng(seed)
    lev = qam_levels(n_lev)
    l64 = lev.astype(np.float64)
    d = float(l64[1] - l64[0])
    pad = 64
    n_tot = K + extra + 2 * pad
    iI, iQ = rng.integers(0, n_lev, n_tot), rng.integers(0, n_lev, n_tot)
    s = l64[iI] + 1j * l64[iQ]
    m = np.arange(K + extra)
    track = gain * (1j ** rot) * s[pad + m - lag]
    track = track + gain * pert * d * (rng.uniform(-1, 1, K + extra) + 1j * rng.uniform(-1, 1, K + extra))
    tI, tQ = iI[pad:pad + K].copy(), iQ[pad:pad + K].copy()
    injected = np.sort(rng.choice(np.arange(40, K - 70), n_err, replace=False)) if n_err else np.zeros(0, np.int64)
    for q, p in enumerate(injected):                                   # a neighbour on one axis, inward at the edge levels
        ax = tI if q % 2 == 0 else tQ
        ax[p] += 1 if ax[p] == 0 or (ax[p] < n_lev - 1 and q % 4 < 2) else -1
    data = np.stack([lev[tI], lev[tQ]]).astype(np.float16)
    res = dict(track=track, data=data, levels=lev, injected=injected, rx=None, h=None)
    if validator is not None:
        sps, M, side = validator
        mh = M // 2
        c = 0.8 * np.exp(0.1j)
        hc = np.zeros(M, complex)
        hc[mh] = c
        if side and mh >= sps:
            hc[mh - sps], hc[mh + sps] = side * d * (1 - 0.5j), side * d * (-0.6 + 0.3j)
        kk = cma_symbol_indices(K * sps, sps, M)                       # symbol j lands at kk[j]
        x = np.zeros(K * sps, complex)
        x[::sps] = track[kk] / c
        res["rx"] = np.stack([x.real, x.imag]).astype(np.float32)
        res["h"] = np.stack([hc.real, hc.imag]).astype(np.float32)
    return res


def shift_conditions(cI, cQ, branch, length):
    """(winning |corr| / runner-up on its rail, distance of the deciding comparison from the 0.02 * length threshold relative to it)."""
    win = cQ if branch == "Q" else cI
    s = np.sort(win)[::-1]
    ratio = s[0] / s[1] if len(s) > 1 and s[1] > 0 else np.inf
    thr = 0.02 * length
    return float(ratio), float(abs(cI.max() - thr) / thr)


def conditioned_dfe_frame(seed, N, n_lev, K2, outliers):
    """ff[N] (complex64), fb[K2] (complex64), init[N] (int8), the expected decisions[N] and TX data [2,N] (fp16) for the recursion:
    ff[p] = symbol[p] - sum_j fb[j] decided[p-1-j] + noise, noise uniform within +-0.3 level spacings per coordinate, `decided` the values the
    recursion decides: the symbol, except at `outliers` positions where ff is displaced by exactly one level spacing on one axis (inward at the
    edge levels) and the neighbouring level is decided -- a wrong decision whose feedback the next K2 steps must carry to stay on the
    expected trajectory.  init holds the true first K2 decisions (the recursion's start) and random indices everywhere else, so every
    speculative warm-up starts from a wrong state."""
    rng = np.random.default_rng(seed)
    lev = qam_levels(n_lev)
    l64 = lev.astype(np.float64)
    d = float(l64[1] - l64[0])
    iI, iQ = rng.integers(0, n_lev, N), rng.integers(0, n_lev, N)
    dI, dQ = iI.copy(), iQ.copy()
    pos = np.sort(rng.choice(np.arange(K2, N), outliers, replace=False)) if outliers else np.zeros(0, np.int64)
    for q, p in enumerate(pos):
        ax = dI if q % 2 == 0 else dQ
        ax[p] += 1 if ax[p] == 0 or (ax[p] < n_lev - 1 and q % 4 < 2) else -1
    decided = l64[dI] + 1j * l64[dQ]
    fb = (rng.uniform(0.15, 0.45, K2) * np.exp(2j * np.pi * rng.uniform(0, 1, K2))).astype(np.complex64)
    fbk = np.zeros(N, complex)
    for j in range(K2):
        fbk[j + 1:] += complex(fb[j]) * decided[:N - 1 - j]
    ff = decided - fbk + 0.3 * d * (rng.uniform(-1, 1, N) + 1j * rng.uniform(-1, 1, N))
    init = rng.integers(0, n_lev * n_lev, N)
    init[:K2] = (dI * n_lev + dQ)[:K2]
    data = np.stack([lev[iI], lev[iQ]]).astype(np.float16)
    return dict(ff=ff.astype(np.complex64), fb=fb, init=init.astype(np.int8), expected=dI * n_lev + dQ, data=data, levels=lev, outliers=pos)


def shifted_data(data, lag, seed=0):
    """TX data moved so that find_shift_symb reports `lag` against the unmoved track: data'[m] = data[m + lag], random levels at the ends."""
    rng = np.random.default_rng(seed)
    N = data.shape[1]
    lv = np.unique(data)
    out = lv[rng.integers(0, len(lv), (2, N))]
    src = np.arange(N) + lag
    ok = (src >= 0) & (src < N)
    out[:, ok] = data[:, src[ok]]
    return out.astype(np.float16)


# ------------------------------------------------------------------------------------------------------------------ the cases both test modules walk
def cma_grid():
    """(M, sps, K) of the lr = 0 grid: both sides of the M <= 31 split and the ends of the tap range, sps with joff = 0 (1), the script's (2)
    and others, K at the smallest legal value (M), below the look-ahead of 8, around the 64-symbol flush and its second round."""
    shapes = []
    for M in (1, 3, 29, 31, 33, 61, 63):
        for sps in (1, 2, 3, 4, 8):
            for K in sorted({M, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 300, 1000}):
                if K >= M:
                    shapes.append((M, sps, K))
    return shapes


# seed, K, n_lev, rot, lag, n_err, n_shift, sps, M, side taps, gain, intended branch
def validator_cases():
    """Conditioned frames of the CMA validation kernel, grouped into batches of one shape: every lag of n_shift = 21 and 23 (but -11, where
    the reference's slice is empty), n_shift = 1, the four rotations, n_lev 2 / 4 / 8, and the three branches of the shift search."""
    batches = []
    for n_lev, n_shift, sps, M, K in ((2, 21, 2, 31, 4000), (4, 23, 1, 33, 4001), (8, 21, 3, 63, 3500)):
        hsh = n_shift // 2
        lags = [g for g in range(-hsh, hsh + 1) if not (n_shift == 23 and g == -11)]
        runs = [dict(seed=100 * n_lev + i, lag=g, rot=i % 4, n_err=3 + i % 5, side=0.03 if i % 2 else 0.0, gain=1.0) for i, g in enumerate(lags)]
        batches.append(dict(K=K, n_lev=n_lev, n_shift=n_shift, sps=sps, M=M, runs=runs,
                            branches=["Q" if r["rot"] % 2 else "I" for r in runs]))
    batches.append(dict(K=1001, n_lev=4, n_shift=1, sps=2, M=1, branches=["I", "I"],
                        runs=[dict(seed=901 + i, lag=0, rot=2 * i, n_err=2 + i, side=0.0, gain=1.0) for i in range(2)]))
    batches.append(dict(K=26000, n_lev=2, n_shift=21, sps=1, M=31, branches=["I kept", "Q"],       # 0.02 K = 520 > 990 / 2 gain
                        runs=[dict(seed=950, lag=-4, rot=2, n_err=6, side=0.0, gain=0.8), dict(seed=951, lag=7, rot=3, n_err=5, side=0.03, gain=0.8)]))
    return batches


def build_validator_batch(b, tries=40):
    """The frames of one batch.  The CPE's own phase estimate wanders by a few hundredths of a radian (much for 64-QAM), which eats into the
    decision margins; each run takes the first seed of seed, seed + 1000, ... whose frame the model evaluates with a margin of at least 1 %
    of a level spacing, the intended shift and exactly the injected errors."""
    frames = []
    for r in b["runs"]:
        for t in range(tries):
            fr = conditioned_eval_frame(r["seed"] + 1000 * t, b["K"], b["n_lev"], r["rot"], r["lag"], r["n_err"], gain=r["gain"],
                                        pert=0.1 if b["n_lev"] == 8 else 0.25, validator=(b["sps"], b["M"], r["side"]))
            v = validate(fr["rx"], fr["h"], fr["data"], fr["levels"], b["sps"], b["n_shift"])
            d = float(fr["levels"][1] - fr["levels"][0])
            if v["shift"] == r["lag"] and v["counts"].min() == r["n_err"] and v["margin"].min() >= 0.01 * d:
                fr["model"] = v
                frames.append(fr)
                break
        else:
            raise RuntimeError(f"no conditioned validator frame for {b['K']}, {r}")
    return frames


def lmmse_cases():
    """(K taps, N, n_cut, n_shift, n_lev) of the LMMSE evaluation, R = 3 frames each with their own taps, rotation and lag."""
    return [(2, 1023, 0, 1, 2), (20, 1043, 0, 21, 4), (64, 1063, 20, 1, 8), (20, 1083, 20, 21, 8), (2, 1065, 21, 1, 4), (64, 1128, 21, 64, 2),
            (20, 3001, 20, 21, 4), (64, 4096, 21, 64, 8), (2, 4097, 0, 21, 2), (20, 4097, 21, 64, 4)]


def lmmse_rx_taps(track, K, r):
    """rx[2,N] f32 and taps[K] complex64 whose compl_conv is `track` (N + 1 samples; sample 0 comes out as 0): an even filter with one
    spike c at tap K / 2 gives out[i] = c x[i - 1]; frames r > 0 get a complex c and small neighbouring taps (a little ISI)."""
    c = 1.0 if r == 0 else 0.9 * np.exp(0.7j * r)
    taps = np.zeros(K, complex)
    taps[K // 2] = c
    if r:
        taps[K // 2 - 1] = 0.02 * c * (1 - 0.5j)
        if K > 2:
            taps[K // 2 + 1] = 0.015 * c * (-0.6 + 1j)
    x = track[1:] / c
    return np.stack([x.real, x.imag]).astype(np.float32), taps.astype(np.complex64)


def lmmse_lag(case, r):
    K, N, n_cut, n_shift, n_lev = case
    hsh = n_shift // 2
    return (-hsh + 1 + (7 * r + K) % (2 * hsh)) if hsh else 0         # never -hsh: with hsh = 11 + n_cut the reference's slice is empty there


def build_lmmse_case(case, r):
    """Frame r of a case -> (frame dict with rx / taps, lag)."""
    K, N, n_cut, n_shift, n_lev = case
    lag = lmmse_lag(case, r)
    rot = 2 * (r % 2) if (N < 2900 and n_shift > 1) else (r + K // 2) % 4      # a short frame's 0.02 N is below the noise of the I rail
    fr = conditioned_eval_frame(1000 * K + N + r, N, n_lev, rot, lag, 4 + r, extra=1, pert=0.15)
    fr["rx"], fr["taps"] = lmmse_rx_taps(fr["track"], K, r)
    return fr, lag


def longer_slice_frame(seed=77, N=1100, K=20, n_cut=20, lag=3):
    """An LMMSE frame (16-QAM, no rotation) in which the one extra track sample of the evaluation slice (:282: L + 1 samples against L of
    the data) is large enough to lower the rescale by about 4 %, and one decided sample sits 1 % of a level spacing inside the boundary
    between levels 2 and 3 WITH that rescale and 3 % outside WITHOUT it; the TX symbol there is level 2.  So the error count is the injected
    one when the extra sample enters the scale and one more when it does not."""
    fr = conditioned_eval_frame(seed, N, 4, 0, lag, 3, extra=1, pert=0.15)
    tr = fr["track"]
    l64 = fr["levels"].astype(np.float64)
    d = float(l64[1] - l64[0])
    r0, L = n_cut + 11 + lag, N - 22 - 2 * n_cut - lag
    tr[r0 + L] = 0.04 * L * np.mean(np.abs(tr[r0:r0 + L])) * np.exp(0.25j * np.pi)
    p = r0 + 500
    fr["data"][0, p - lag] = fr["levels"][2]
    tx = fr["data"].astype(np.float64)[:, n_cut + 11:n_cut + 11 + L]
    for _ in range(3):
        sw = np.mean(np.hypot(tx[0], tx[1])) / np.mean(np.abs(tr[r0:r0 + L + 1]))
        tr[p] = 0.99 * d / sw + 1j * tr[p].imag
    fr["rx"], fr["taps"] = lmmse_rx_taps(tr, K, 0)
    fr["pulled"] = p - r0                                              # index inside the evaluated slice
    return fr


def dfe_run_seeds(n_lev, K2, N):
    """Seeds of the runs that share one vaeq_awgn_dfe call (their own ff, fb taps and init each): four, two for the long frames."""
    return [100 * n_lev + K2 + 1000 * r for r in range(4 if N < 5000 else 2)]


def dfe_cases():
    """(n_lev, K2, N, outliers, [(C, W)]) of the recursion: all six <NL, K2M> instantiations on both sides of the K2 = 4 | 5 split; chunkings:
    serial, CH = K2 exactly, a short last chunk, more chunks requested than non-empty ones, and the cap C = 8192 with CH = K2."""
    cases = []
    for n_lev in (2, 4, 8):
        for K2 in (1, 4, 5, 10):
            N = K2 + 37 * K2 * 3 + 5                                   # C = 37 * 3 + ... chunks of K2; odd sizes
            CH3 = 3 * K2 + 1
            Cs = [(1, 0), (-(-(N - K2) // K2), 0), (-(-(N - K2) // K2), K2 - 1), (-(-(N - K2) // K2), 1), (7, 0), (7, N), (7, -(-(N - K2) // 7) + 3),
                  (-(-(N - K2) // CH3), CH3 + 3), ((N - K2) // 2 + 1 if K2 == 1 else (N - K2) // K2 - 1, 0)]
            cases.append((n_lev, K2, N, 9, Cs))
    cases.append((2, 1, 1 + 8192, 40, [(8192, 0), (8192, 1)]))
    cases.append((4, 1, 1 + 8192, 40, [(8192, 0), (8192, 4)]))
    cases.append((8, 5, 5 + 8192 * 5, 200, [(8192, 0), (8192, 4)]))
    cases.append((4, 10, 10 + 8192 * 10, 300, [(8192, 0), (8192, 9), (8192, 13)]))
    return cases
