"""Two integer models of vaeq_staircase_decode (include/vaeq.h): the sliding-window iterative decoder of a staircase code over shortened BCH
components, acting on the error pattern e = (llr < 0) xor the TX bits under vaeq_ldpc_decode's bit-packed map.

chain()      (a) the specification on bitmaps: e[L + 1, s, s] with block 0 all zero, every component decided by _ref_bch.decode (syndromes,
             Berlekamp-Massey, a root search over all 2^m - 1 positions, the three-status rule) plus the block-0 rule of pair 1, with a counter
             for every branch: _ref_bch.decode's own (status0 / status1 / status2, miscorrected, undetected, L>t, roots<L, shortened-root) and
             block0-root, bad_flips, pos-noflip (a position ended by an iteration without a flip) and pos-cap (ended by `iters`);
chain_syn()  (b) an independent restatement that never builds a locator and never reads a component's bits: 2t syndromes per component, updated on
             every flip, decided by _ref_bch.Table (the unique set of at most t positions with these syndromes, by enumeration); only for codes
             small enough for the table.  tests/test_ref_staircase_host.py holds the two to each other;
errors()     the error pattern of device-layout tensors, [R, C, L, s, s];
decode()     (a) over them: out[R, C, 8], hard[R, C, n_chain], pos_err[R, C, L], pos_iters[R, C, P] and the counters.
"""
import collections

import numpy as np

import _ref_bch as B
import _ref_ldpc as M


def n_positions(L, W):
    return max(1, L - W + 1)


def component(m, t, s, i, positions, count, memo=None):
    """One component of pair i with the error positions `positions` (of 2 s) -> (status, flips): vaeq_bch_outer's rule with n_o = 2 s, and in
    pair 1 a set with a position below s is status 2."""
    if not positions:
        count["status0"] += 1
        return 0, []
    key = (i == 1, tuple(positions))
    if memo is not None and key in memo:
        status, flips, own = memo[key]
    else:
        own = collections.Counter()
        status, flips = B.decode(m, t, 2 * s, positions, own)
        if status == 1 and i == 1 and min(flips) < s:
            own = collections.Counter({"status2": 1, "block0-root": 1})
            status, flips = 2, []
        if memo is not None:
            memo[key] = status, flips, own
    count.update(own)
    return status, flips


def chain(m, t, s, L, W, iters, e, count=None, memo=None):
    """(a).  e[L, s, s] bool, the error pattern of blocks 1 .. L -> (fig = iters, ok, post_err, iters_max, nflip, bad_flips; the final
    e[L, s, s]; pos_err[L]; pos_iters[P])."""
    count = collections.Counter() if count is None else count
    E = np.zeros((L + 1, s, s), bool)
    E[1:] = e
    P = n_positions(L, W)
    pos_iters = np.zeros(P, np.int64)
    ok, nflip, bad = 1, 0, 0
    for q in range(P):
        clean = True
        for it in range(iters):
            flipped, clean = 0, True
            for i in range(q + 1, min(q + W, L) + 1):
                word = np.concatenate([E[i - 1].T, E[i]], axis=1)              # [s, 2 s]: component j = [column j of block i - 1 | row j of block i]
                todo = []
                for j in np.nonzero(word.any(axis=1))[0]:
                    status, flips = component(m, t, s, i, [int(p) for p in np.nonzero(word[j])[0]], count, memo)
                    clean &= status == 0
                    todo += [(int(j), p) for p in flips]
                count["status0"] += s - int(word.any(axis=1).sum())
                for j, p in todo:                                              # all decided on the state before the step, then applied
                    blk, a, b = (i - 1, p, j) if p < s else (i, j, p - s)
                    assert blk > 0
                    bad += not E[blk, a, b]
                    E[blk, a, b] ^= True
                flipped += len(todo)
            pos_iters[q] = it + 1
            nflip += flipped
            if not flipped:
                count["pos-noflip"] += 1
                break
        else:
            count["pos-cap"] += 1
        ok &= int(clean)
    count["bad_flips"] += bad
    assert not E[0].any()
    pos_err = E[1:].sum(axis=(1, 2))
    return (int(pos_iters.sum()), ok, int(pos_err.sum()), int(pos_iters.max()), nflip, bad), E[1:], pos_err, pos_iters


def chain_syn(m, t, s, L, W, iters, e, table=None):
    """(b).  The same figures from per-component syndromes alone: -> (fig, the final e[L, s, s], pos_err[L], pos_iters[P])."""
    T = B.Table(m, t, 2 * s) if table is None else table
    zero = (0,) * (2 * t)
    err = {(i + 1, int(a), int(b)) for i, a, b in zip(*np.nonzero(e))}         # the coordinates (block, row, column) of the errors now
    syn = {(i, j): zero for i in range(1, L + 1) for j in range(s)}

    def touch(blk, a, b):                                                       # bit (a, b) of block blk changes: two components see it
        for key, p in (((blk, a), s + b), ((blk + 1, b), a)):
            if key in syn:
                syn[key] = tuple(x ^ y for x, y in zip(syn[key], T.col[p]))

    for c in err:
        touch(*c)
    P = n_positions(L, W)
    pos_iters = np.zeros(P, np.int64)
    ok, nflip, bad = 1, 0, 0
    for q in range(P):
        it, clean = 0, True
        while it < iters:
            it += 1
            flipped, clean = 0, True
            for i in range(q + 1, min(q + W, L) + 1):
                todo = []
                for j in range(s):
                    sy = syn[i, j]
                    if sy == zero:
                        continue
                    clean = False
                    pos = T.table.get(sy)
                    if pos is None or (i == 1 and pos[0] < s):                  # (the table's sets are ascending)
                        continue
                    todo += [(i - 1, p, j) if p < s else (i, j, p - s) for p in pos]
                for c in todo:
                    bad += c not in err
                    err ^= {c}
                    touch(*c)
                flipped += len(todo)
            nflip += flipped
            if not flipped:
                break
        pos_iters[q] = it
        ok &= int(clean)
    E = np.zeros((L + 1, s, s), bool)
    for c in err:
        E[c] = True
    pos_err = E[1:].sum(axis=(1, 2))
    return (int(pos_iters.sum()), ok, int(pos_err.sum()), int(pos_iters.max()), nflip, bad), E[1:], pos_err, pos_iters


def errors(llr, bits, t0, C, L, s):
    """llr[R, w, N] float32 and bits[R, w, N] int8 -> (e[R, C, L, s, s] bool, tx[R, C, L s^2] bool, erased[R, C]): a NaN and +-0 are bit 0."""
    n = L * s * s
    x, tx = M.codewords(llr, t0, C, n), M.codewords(bits, t0, C, n).astype(bool)
    with np.errstate(invalid="ignore"):
        e = (x < 0) != tx
    return e.reshape(llr.shape[0], C, L, s, s), tx, (x == 0).sum(-1)


def decode(llr, bits, m, t, s, L, W, iters, t0, C, count=None, memo=None):
    """(a) over device-layout tensors -> (out[R, C, 8] int64, hard[R, C, n_chain] int8, pos_err[R, C, L], pos_iters[R, C, P], the Counter)."""
    count = collections.Counter() if count is None else count
    memo = {} if memo is None else memo
    e, tx, erased = errors(llr, bits, t0, C, L, s)
    R, P = llr.shape[0], n_positions(L, W)
    out, hard = np.zeros((R, C, 8), np.int64), np.zeros((R, C, L * s * s), np.int8)
    pos_err, pos_iters = np.zeros((R, C, L), np.int64), np.zeros((R, C, P), np.int64)
    for r in range(R):
        for c in range(C):
            (it, ok, post, most, nflip, bad), fin, pos_err[r, c], pos_iters[r, c] = chain(m, t, s, L, W, iters, e[r, c], count, memo)
            out[r, c] = it, ok, post, int(e[r, c].sum()), erased[r, c], most, nflip, bad
            hard[r, c] = tx[r, c] ^ fin.reshape(-1)
    return out, hard, pos_err, pos_iters, count
