"""vaeq_chase_bch_decode through engine.chase_decode with an EbchCode against model (1) of tests/_ref_ebch.py, bit for bit: out[R, C, 6] and both
tensors of the payload stream with np.array_equal, no tolerance -- the rule is integers and float32 additions in a fixed order.  The model finds
the located positions by Berlekamp-Massey and a root search, the kernel by a closed form.  The cases are tests/_ebch_cases.py's (its docstring
says what they hold and tests/test_ref_ebch_host.py that they reach every branch of the rule): ten codes from the plain (15, 7) to the extended
(256, 239), one to four lane slots, patterns 0, 1, 4 and 6, w in {1, 4, 12}, the bit-packed map and the interleaver at depth 2 (ragged) and C,
K < n and K = n, both spreads, t0 in {0, 5}, ties, a NaN, +-0 and +-inf, loud wrong bits around the used span.  Then more words than a tile,
more tiles than the launch has workgroups, two calls against each other with the stream absent, and the defaults."""
import numpy as np
import pytest
import torch

import _ebch_cases as K
import _ref_chase as X
import _ref_ebch as E

pytestmark = pytest.mark.gpu

FIGS = ("status", "pre_err", "bit_err", "nflip", "erased", "pay_err")


def _code(name):
    from vae_equalizer_amd.engine import EbchCode
    c = K.CODES[name]
    code = EbchCode(c.m, c.n, bool(c.ext))
    assert (code.n, code.n_i, code.k, code.extended) == (c.n, c.n_i, c.k, bool(c.ext))
    return code


def _run(case, llr, bits, **over):
    from vae_equalizer_amd.engine import chase_decode
    kw = dict(t0=case.t0, codewords=case.C, depth=case.depth or None, patterns=case.p, payload=case.K, spread=bool(case.spread), want_stream=True)
    kw.update(over)
    ret = chase_decode(torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda(), _code(case.code), **kw)
    torch.cuda.synchronize()
    return ret


def _out(ret):
    return np.stack([ret[k].cpu().numpy() for k in FIGS], -1)


def _check(ret, want, n, Kp, tag):
    out, s_llr, s_bits, _ = want
    got = _out(ret)
    g_llr, g_bits = ret["stream"]["llr"].cpu().numpy(), ret["stream"]["bits"].cpu().numpy()
    print(f"{tag}: status {np.bincount(out[..., 0].ravel(), minlength=3).tolist()} pre_err {int(out[..., 1].sum())} post_err {int(out[..., 2].sum())} "
          f"flips {int(out[..., 3].sum())} erased {int(out[..., 4].sum())} pay_err {int(out[..., 5].sum())}; out differs in {int((got != out).sum())}, "
          f"stream llr in {int((g_llr[:, 0] != s_llr).sum())}, stream bits in {int((g_bits[:, 0] != s_bits).sum())} of {s_bits.size}")
    assert got.dtype == np.int64 and g_llr.dtype == np.float32 and g_bits.dtype == np.int8
    assert g_llr.shape == (out.shape[0], 1, s_llr.shape[1]) and g_bits.shape == g_llr.shape
    assert np.array_equal(got, out)
    assert np.array_equal(g_llr[:, 0], s_llr) and np.array_equal(g_bits[:, 0], s_bits)
    for k, v in X.figures(out, n, Kp).items():
        assert np.array_equal(ret[k].cpu().numpy(), v), k


@pytest.mark.parametrize("case", K.CHASE, ids=lambda c: c.name)
def test_chase_bch_matches_model(case):
    llr, bits = K.chase_tensors(case)
    _check(_run(case, llr, bits), K.chase_expected(case), K.CODES[case.code].n, case.K, case.name)


def test_several_tiles_per_run():
    case = K.CHASE_TILES
    llr, bits = K.chase_tensors(case)
    _check(_run(case, llr, bits), K.chase_expected(case), K.CODES[case.code].n, case.K, case.name)


def test_grid_stride():
    case = K.CHASE_STRIDE
    llr, bits = K.chase_tensors(case)
    _check(_run(case, llr, bits), K.chase_expected(case), K.CODES[case.code].n, case.K, case.name)


@pytest.mark.parametrize("case", [K.CHASE[i] for i in (2, 7, 14, len(K.CHASE) - 1)], ids=lambda c: c.name)
def test_repeatable_and_stream_optional(case):
    llr, bits = K.chase_tensors(case)
    a, b, c = _run(case, llr, bits), _run(case, llr, bits), _run(case, llr, bits, want_stream=False)
    assert "stream" not in c and set(a) - set(c) == {"stream"}
    assert np.array_equal(_out(a), _out(b)) and np.array_equal(_out(a), _out(c))
    for k in ("llr", "bits"):
        assert torch.equal(a["stream"][k], b["stream"][k])
    for k in c:
        assert torch.equal(a[k], c[k]), k


def test_defaults():
    from vae_equalizer_amd.engine import chase_decode, ebch_code
    case = next(c for c in K.CHASE if c.depth == 0 and c.w == 12 and c.code == "b15")   # three spare symbols of 12 bits behind the C words
    llr, bits = K.chase_tensors(case)
    code = ebch_code(4, extended=False)
    fit = (llr.shape[-1] - case.t0) * case.w // code.n
    assert fit > case.C and (code.n, code.k) == (15, 7) and (ebch_code(5).n, ebch_code(5).k, ebch_code(8, n=201).n_i) == (32, 21, 200)
    ret = chase_decode(torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda(), code, t0=case.t0, want_stream=True)
    want = E.decode_chase(llr, bits, K.CODES["b15"], 4, code.k, case.t0, fit, 0, 1)   # every word that fits, patterns 4, payload k, spread
    _check(ret, want, code.n, code.k, "defaults")
