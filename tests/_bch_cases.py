"""What tests/test_bch_gpu.py and tests/test_bch_envelope_gpu.py share: synthetic `post` and `bits` tensors with error patterns planted through
the stream map and the TX-bit map, the call into engine.bch_outer, and the comparison with tests/_ref_bch.py that asserts out, loc and the
derived figures with np.array_equal after printing them.

make_case()          the weights (a + r C_o) % (2t + 3) of tests/test_bch_gpu.py at seeded positions;
plant_case()         a given list of error patterns, one per outer codeword;
_run, _out, _check   the call with want_loc, out[R, C_o, 4] of its result, the assertions.
"""
import numpy as np
import torch

import _ref_bch as B
import _ref_ldpc as M
import _ref_ldpc_il as IL


def _frame(rng, R, C, n, w, t0, depth):
    """-> (bits[R, w, N] int8 random, tx[R, C, n] bool under the map): N leaves not one symbol to spare behind the interleaver, three bit-packed."""
    N = t0 + C * IL.symbols_per_codeword(n, w) if depth else t0 + -(-C * n // w) + 3
    bits = rng.integers(0, 2, (R, w, N)).astype(np.int8)
    tx = (IL.codewords_il(bits, t0, C, n, depth) if depth else M.codewords(bits, t0, C, n)).astype(bool)
    return bits, tx


def _post(rng, rx, i16, special):
    """rx[R, C, n] bool, the received bits -> post float32 or int16 with rx = post < 0; int16 with -32768 and 0 among the values; special: a NaN,
    a +0 and a -0 per run on received zeros (all of them bit 0)."""
    R, C, n = rx.shape
    if i16:
        post = rng.integers(1, 128, (R, C, n)).astype(np.int16)
        post = np.where(rx, -post, post).astype(np.int16)
        post[rx & (rng.random((R, C, n)) < 0.1)] = -32768
        post[~rx & (rng.random((R, C, n)) < 0.1)] = 0
    else:
        post = rng.uniform(0.5, 20.0, (R, C, n)).astype(np.float32)
        post = np.where(rx, -post, post).astype(np.float32)
        if special:
            for r in range(R):
                z = np.flatnonzero(~rx[r].ravel())
                pick = rng.choice(z, 3, replace=False)
                post[r].ravel()[pick] = np.array([np.nan, 0.0, -0.0], np.float32)
    return post


def make_case(seed, R, C, n, w, t0, depth, code, K, spread, C_o, i16=False, special=False):
    """-> (post[R, C, n] float32 or int16, bits[R, w, N] int8): random TX bits; outer codeword a of run r carries (a + r C_o) % (2t + 3) errors at
    seeded positions, but the first outer codeword of run 0 carries a non-zero codeword of the shortened code where there is one; every position
    outside the outer codewords is in error with probability 1/2.  N leaves not one symbol to spare behind the interleaver, three bit-packed.
    special: a NaN, a +0 and a -0 per run on received zeros (all of them bit 0)."""
    m, t, n_o = code
    rng = np.random.default_rng(seed)
    bits, tx = _frame(rng, R, C, n, w, t0, depth)
    c, i = B.stream_map(C_o, n_o, K, spread)
    e = rng.integers(0, 2, (R, C, n)).astype(bool)             # loud wherever no outer codeword lives
    word = B.codeword_of(m, t, n_o)
    for r in range(R):
        pat = np.zeros((C_o, n_o), bool)
        for a in range(C_o):
            wt = min((a + r * C_o) % (2 * t + 3), n_o)
            pos = word if r == 0 and a == 0 and word is not None else rng.choice(n_o, wt, replace=False)
            pat[a, pos] = True
        e[r][c, i] = pat
    return _post(rng, tx ^ e, i16, special), bits


def plant_case(seed, R, C, n, w, t0, depth, code, K, spread, C_o, patterns, i16=False, special=False):
    """As make_case, but outer codeword a of run r carries patterns[r C_o + a], a list of positions below n_o (len(patterns) == R C_o)."""
    n_o = code[2]
    assert len(patterns) == R * C_o
    rng = np.random.default_rng(seed)
    bits, tx = _frame(rng, R, C, n, w, t0, depth)
    c, i = B.stream_map(C_o, n_o, K, spread)
    e = rng.integers(0, 2, (R, C, n)).astype(bool)             # loud wherever no outer codeword lives
    pat = np.zeros((R * C_o, n_o), bool)
    for g, pos in enumerate(patterns):
        pat[g, pos] = True
    e[:, c, i] = pat.reshape(R, C_o, n_o)
    return _post(rng, tx ^ e, i16, special), bits


def _run(post, bits, code, n, C_o, **kw):
    from vae_equalizer_amd.engine import BchCode, bch_outer
    m, t, n_o = code
    r = bch_outer(torch.from_numpy(post).cuda(), torch.from_numpy(bits).cuda(), BchCode(m, t, n_o), n, codewords=C_o, want_loc=True, **kw)
    torch.cuda.synchronize()
    return r


def _out(r):
    return np.stack([r[k].cpu().numpy() for k in ("status", "pre_err", "bit_err", "nflip")], -1)


def _check(r, want_out, want_loc, n_o, tag):
    got_out, got_loc = _out(r), r["loc"].cpu().numpy()
    print(f"{tag}: status {np.bincount(want_out[..., 0].ravel(), minlength=3).tolist()} pre_err {int(want_out[..., 1].sum())} "
          f"post_err {int(want_out[..., 2].sum())} flips {int(want_out[..., 3].sum())}; out differs in {int((got_out != want_out).sum())}, "
          f"loc in {int((got_loc != want_loc).sum())} of {want_loc.size}")
    assert got_out.dtype == np.int64 and got_loc.dtype == np.int16 and got_loc.shape == want_loc.shape
    assert np.array_equal(got_out, want_out)
    assert np.array_equal(got_loc, want_loc)
    for k, v in B.figures(want_out, n_o).items():
        assert np.array_equal(r[k].cpu().numpy(), v), k
