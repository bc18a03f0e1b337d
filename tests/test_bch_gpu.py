"""vaeq_bch_outer (the hard-decision outer BCH decoder behind the LDPC decoders) against the integer model tests/_ref_bch.py, through
engine.bch_outer and engine.ldpc_decode(outer=...).

No tolerance: the decoder is integer arithmetic and the header states its rule without an algorithm, so out[R, C_o, 4] and loc[R, C_o, t] have to
be the model's.  tests/test_ref_bch_host.py pins the model to the rule by enumeration and shows that every branch binds.

The inputs are synthetic `post` and `bits` tensors, no LDPC run: per outer codeword an error pattern of weight 0 .. 2t + 2 planted through the
stream map (and so through the LDPC decoder's own bit map), one outer codeword of every code that has one carrying a non-zero codeword of the
shortened code, and errors at every other bit in every position that belongs to no outer codeword -- past the payload of an LDPC codeword and
past C_o n_o in the stream -- which must not count.  Cases: R = 3 runs of C = 5 codewords of n = 42 bits (the array_code(3, 6, 7) geometry), w in
{12, 8}, t0 in {0, 11}, depth in {None, 1, 2, 5}; inside each, the codes BchCode(4, 2), BchCode(4, 3, n=11) and BchCode(4, 1), K in {28, 42}, the
spread on and off, post as float32 and as int16.  (m, t) = (4, 3) has 10 parity bits, so n = 11 is the shortest code the envelope admits: four
shortened positions for the locator's roots to fall on; n = 9, which the model-only tests keep, is refused by the entry point
(tests/test_abi_refusals_bch_host.py).  BchCode(4, 1) is a perfect code and never reaches status 2, so every status, a miscorrection, an
undetected error and every branch of the rule are asserted over the three codes of a parametrisation together.  Then n = 744 with BchCode(8, 4),
the corner of the envelope (m = 13, t = 16, n_o = 8191), offsets past 2^32, repeatability, ldpc_decode(outer=...) on real LLRs, the chunked fec_figures and the ValueErrors.  Every test prints its figures before it asserts.  make_case, _run, _out and _check live in tests/_bch_cases.py;
the other fields, the ladder of t, the shortenings and several codewords per wave are tests/test_bch_envelope_gpu.py's."""
import collections

import numpy as np
import pytest
import torch

import _ref_bch as B
import _ref_ldpc as M
import _ref_ldpc_il as IL
from _bch_cases import _check, _out, _run, make_case

pytestmark = pytest.mark.gpu

CODES = ((4, 2, 15), (4, 3, 11), (4, 1, 15))                # (m, t, n_o)


def _codewords(C, K, n_o):
    """The most outer codewords that leave stream bits behind them: those bits are loud and must not count."""
    return (C * K - 1) // n_o


@pytest.mark.parametrize("depth", [None, 1, 2, 5])
@pytest.mark.parametrize("t0", [0, 11])
@pytest.mark.parametrize("w", [12, 8])
def test_against_the_model(w, t0, depth):
    R, C, n = M.R_, M.C_, 42
    total = collections.Counter()
    for ci, code in enumerate(CODES):
        for K in (28, 42):
            C_o = _codewords(C, K, code[2])
            assert C_o * code[2] < C * K and R * C_o >= 2 * code[1] + 3
            for spread in (0, 1):
                for i16 in (False, True):
                    seed = 100000 + 1000 * (w + t0 + (depth or 0) * 31) + 100 * ci + 10 * (K == 42) + 2 * spread + i16
                    post, bits = make_case(seed, R, C, n, w, t0, depth, code, K, spread, C_o, i16, special=not i16 and spread == 1)
                    want_out, want_loc, count = B.outer(post, bits, *code, C_o, K, spread, t0, depth)
                    total.update(count)
                    r = _run(post, bits, code, n, C_o, t0=t0, depth=depth, payload=K, spread=bool(spread))
                    _check(r, want_out, want_loc, code[2], f"w={w} t0={t0} depth={depth} code={code} K={K} spread={spread} int16={i16}")
                    if not i16 and spread == 1:
                        assert np.isnan(post).sum() == R and (post == 0).sum() == 2 * R
    print(dict(total))
    for k in ("status0", "status1", "status2", "miscorrected", "undetected", "roots<L", "shortened-root", "L>t"):
        assert total[k] > 0, k


@pytest.mark.parametrize("spread", [0, 1])
@pytest.mark.parametrize("depth", [None, 2])
def test_n744_bch_8_4(depth, spread):
    """array_code(4, 24, 31)'s geometry: n = 744, K = 620, C = 5, BchCode(8, 4): C_o = 12 outer codewords of 255 bits, four iterations of the
    lanes per codeword, the last one ragged."""
    R, C, n, K, w, t0, code = 2, 5, 744, 620, 12, 11, (8, 4, 255)
    C_o = C * K // code[2]
    assert C_o == 12 and C_o * code[2] < C * K
    post, bits = make_case(2000 + 10 * (depth or 0) + spread, R, C, n, w, t0, depth, code, K, spread, C_o, special=True)
    want_out, want_loc, count = B.outer(post, bits, *code, C_o, K, spread, t0, depth)
    print(dict(count))
    assert count["status0"] and count["status1"] and count["status2"] and count["undetected"]
    from vae_equalizer_amd.engine import BchCode, bch_outer
    r = bch_outer(torch.from_numpy(post).cuda(), torch.from_numpy(bits).cuda(), BchCode(8, 4), n, t0=t0, depth=depth, payload=K, spread=bool(spread),
                  want_loc=True)                            # codewords by default: C K // n_o
    torch.cuda.synchronize()
    _check(r, want_out, want_loc, code[2], f"n=744 depth={depth} spread={spread}")


@pytest.mark.parametrize("what", ["t", "t+2", "codeword", "clean"])
def test_corner_of_the_envelope(what):
    """R = 1, C = 2, n = 5064, K = 4220, BchCode(13, 16): one outer codeword of 8191 bits, the largest field, the most syndromes, 128 iterations
    of the lanes; 16 errors are corrected, 18 are not, a codeword of the code passes unseen."""
    R, C, n, K, w, t0, code = 1, 2, 5064, 4220, 12, 0, (13, 16, 8191)
    rng = np.random.default_rng(77)
    N = -(-C * n // w)
    bits = rng.integers(0, 2, (R, w, N)).astype(np.int8)
    tx = M.codewords(bits, t0, C, n).astype(bool)
    c, i = B.stream_map(1, 8191, K, 1)
    e = rng.integers(0, 2, (R, C, n)).astype(bool)
    pat = np.zeros((1, 8191), bool)
    pos = {"t": rng.choice(8191, 16, replace=False), "t+2": rng.choice(8191, 18, replace=False), "clean": [],
           "codeword": B.codeword_of(*code) if what == "codeword" else None}[what]
    pat[0, pos] = True
    e[0][c, i] = pat
    post = np.where(tx ^ e, np.float32(-3.0), np.float32(3.0)).astype(np.float32)
    want_out, want_loc, count = B.outer(post, bits, *code, 1, K, 1, t0, None)
    print(what, dict(count), want_out.tolist())
    assert count[{"t": "status1", "t+2": "status2", "codeword": "undetected", "clean": "status0"}[what]] == 1
    r = _run(post, bits, code, n, 1, t0=t0, payload=K)
    _check(r, want_out, want_loc, 8191, f"corner {what}")
    if what == "t":
        assert want_out[0, 0].tolist() == [1, 16, 0, 16] and np.array_equal(want_loc[0, 0], np.sort(pos))


@pytest.mark.parametrize("depth", [None, 1, 5])
def test_offsets_past_32_bits(depth):
    """w N = 2^33 with the codewords in the last symbols of the frame: the offsets inside a run's bits pass 2^32, the kernel's 64-bit form.  The
    frame is zeros but for its tail (8 GiB on the device, nothing of that size on the host); the model sees the tail alone, at t0 = 0."""
    R, C, n, K, w, N, code, spread = 1, M.C_, 42, 28, 64, 1 << 27, CODES[0], 1
    C_o = _codewords(C, K, code[2])
    post, tail = make_case(9000 + (depth or 0), R, C, n, w, 0, depth, code, K, spread, C_o)
    want_out, want_loc, count = B.outer(post, tail, *code, C_o, K, spread, 0, depth)
    assert count["status1"] and count["status2"] and count["undetected"]
    from vae_equalizer_amd.engine import BchCode, bch_outer
    bits = torch.zeros(R, w, N, dtype=torch.int8, device="cuda")
    t0 = N - tail.shape[2]
    bits[:, :, t0:] = torch.from_numpy(tail).cuda()
    assert (w - 1) * N + t0 > 1 << 32
    r = bch_outer(torch.from_numpy(post).cuda(), bits, BchCode(*code), n, t0=t0, depth=depth, payload=K, codewords=C_o, want_loc=True)
    torch.cuda.synchronize()
    del bits
    _check(r, want_out, want_loc, code[2], f"offsets past 2^32, depth={depth}")


def test_two_calls_give_identical_bits():
    code, K = CODES[0], 28
    C_o = _codewords(M.C_, K, code[2])
    post, bits = make_case(5, M.R_, M.C_, 42, 12, 11, 2, code, K, 1, C_o)
    a, b = (_run(post, bits, code, 42, C_o, t0=11, depth=2, payload=K) for _ in range(2))
    assert np.array_equal(_out(a), _out(b)) and np.array_equal(a["loc"].cpu().numpy(), b["loc"].cpu().numpy())
    from vae_equalizer_amd.engine import BchCode, bch_outer
    e = bch_outer(torch.zeros(0, 5, 42).cuda(), torch.zeros(0, 12, 29, dtype=torch.int8).cuda(), BchCode(4, 2), 42, t0=11, payload=K)
    assert e["status"].shape == (0, 9) and e["BER_outer"].shape == (0,)             # an empty batch: no launch


@pytest.mark.parametrize("quant", [None, dict(bits=5)], ids=["float", "q5"])
@pytest.mark.parametrize("depth", [None, 2])
def test_ldpc_decode_outer_on_real_llrs(depth, quant):
    """ldpc_decode(outer=...) equals bch_outer on the decoder's own post, and the model on that post: float and fixed-point, both maps."""
    from vae_equalizer_amd.engine import BchCode, LdpcCode, bch_outer, ldpc_decode
    name, w, t0 = "array-3-6-7", 12, 11
    shifts, Z = M.CODES[name]
    llr, bits = IL.case(name, w, t0, 2, depth) if depth else M.case(name, w, t0, 2)   # sigma = 0.8: the decoder leaves errors behind
    dl, db = torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda()
    code = BchCode(4, 2)
    kw = dict(t0=t0, codewords=M.C_, depth=depth, quant=quant)
    r = ldpc_decode(dl, db, LdpcCode(shifts, Z), want_post=True, outer=dict(code=code), **kw)
    plain = ldpc_decode(dl, db, LdpcCode(shifts, Z), want_post=True, **kw)
    quiet = ldpc_decode(dl, db, LdpcCode(shifts, Z), outer=dict(code=code), **kw)
    assert set(r) == set(plain) | {"outer"} and set(quiet) == set(r) - {"post"}
    assert all(torch.equal(r[k], plain[k]) for k in plain if torch.is_tensor(plain[k]))
    K, C_o = 21, 5 * 21 // 15                                # the default payload (nb - mb) Z, and all the outer codewords that fit
    post = r["post"].cpu().numpy()
    assert post.dtype == (np.float32 if quant is None else np.int16)
    want_out, want_loc, count = B.outer(post, bits, 4, 2, 15, C_o, K, 1, t0, depth)
    print(f"depth={depth} quant={quant}:", dict(count), "LDPC bit_err", r["bit_err"].sum().item())
    assert np.array_equal(_out(r["outer"]), want_out) and np.array_equal(_out(quiet["outer"]), want_out)
    own = bch_outer(r["post"], db, code, 42, t0=t0, depth=depth, payload=K, want_loc=True)
    _check(own, want_out, want_loc, 15, "bch_outer on the decoder's post")
    assert int(want_out[..., 1].sum()) > 0                  # residual errors in the payload for the outer code to see
    other = ldpc_decode(dl, db, LdpcCode(shifts, Z), outer=dict(code=BchCode(4, 3, 11), payload=42, spread=False, codewords=18), **kw)["outer"]
    want2, _, _ = B.outer(post, bits, 4, 3, 11, 18, 42, 0, t0, depth)
    assert np.array_equal(_out(other), want2)


def test_fec_figures_in_chunks(monkeypatch):
    """With OUTER_POST_BYTES small enough for one run per chunk (three chunks at R = 3), fec_figures returns the unchunked figures."""
    from vae_equalizer_amd import fec as E                     # the module fec_figures resolves ldpc_decode and OUTER_POST_BYTES in
    name, w, t0 = "array-3-6-7", 12, 11
    shifts, Z = M.CODES[name]
    llr, bits = M.case(name, w, t0, 2)
    d = dict(llr=torch.from_numpy(llr).cuda(), bits=torch.from_numpy(bits).cuda())
    calls = []
    real = E.ldpc_decode
    monkeypatch.setattr(E, "ldpc_decode", lambda L, *a, **k: calls.append(L.shape[0]) or real(L, *a, **k))
    for quant in (None, dict(bits=5)):
        fec = dict(code=E.LdpcCode(shifts, Z), t0=t0, quant=quant, outer=dict(code=E.BchCode(4, 2)))
        assert E.OUTER_POST_BYTES == 256 << 20
        del calls[:]
        whole = E.fec_figures(d, fec)
        assert calls == [3]
        monkeypatch.setattr(E, "OUTER_POST_BYTES", 5 * 42 * (4 if quant is None else 2))
        del calls[:]
        parts = E.fec_figures(d, fec)
        assert calls == [1, 1, 1]
        monkeypatch.setattr(E, "OUTER_POST_BYTES", 256 << 20)
        assert set(parts) == set(whole) and set(parts["outer"]) == set(whole["outer"]) and "post" not in parts
        for a, b in ((parts, whole), (parts["outer"], whole["outer"])):
            for k, v in b.items():
                if torch.is_tensor(v):
                    assert a[k].shape == v.shape and torch.equal(a[k], v), k
        assert parts.get("quant") == whole.get("quant")
        del calls[:]
        E.fec_figures(d, {k: v for k, v in fec.items() if k != "outer"})
        assert calls == [3]                                 # without an outer code: one call, as before


def test_value_errors():
    from vae_equalizer_amd import engine as E
    name, w, t0 = "array-3-6-7", 12, 11
    shifts, Z = M.CODES[name]
    llr, bits = M.case(name, w, t0, 1)
    dl, db, code = torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda(), E.LdpcCode(shifts, Z)
    for bad in (dict(), dict(code=code), dict(code=E.BchCode(4, 2), depth=2), dict(code=E.BchCode(4, 2), payload=0), dict(code=E.BchCode(4, 2), payload=43),
                "bch", dict(code=(4, 2))):
        with pytest.raises(ValueError):
            E.ldpc_decode(dl, db, code, t0=t0, outer=bad)
        with pytest.raises(ValueError):
            E.check_fec(dict(code=code, outer=bad))
    with pytest.raises(ValueError):                         # 255 bits do not fit into the 5 x 21 payload bits of a run
        E.ldpc_decode(dl, db, code, t0=t0, outer=dict(code=E.BchCode(8, 4)))
    post = torch.zeros(3, 5, 42).cuda()
    with pytest.raises(ValueError):
        E.bch_outer(post, db, E.BchCode(8, 4), 42, t0=t0)
    with pytest.raises(ValueError):
        E.bch_outer(post, db, (4, 2), 42, t0=t0)
    with pytest.raises(ValueError):
        E.bch_outer(post, db, E.BchCode(4, 2), 41, t0=t0)
    with pytest.raises(ValueError):
        E.bch_outer(post.double(), db, E.BchCode(4, 2), 42, t0=t0)
    with pytest.raises(ValueError):
        E.BchCode(4, 2, 8)
    E.check_fec(dict(code=code, outer=dict(code=E.BchCode(4, 2), payload=28, spread=False, codewords=3)))
    assert E.FEC_KEYS[-1] == "outer"
