"""vaeq_chase_decode through engine.chase_decode against the model of tests/_ref_chase.py, bit for bit: out[R, C, 6] and both tensors of the payload
stream with np.array_equal, no tolerance -- the rule is integers and float32 additions in a fixed order.  The cases are tests/_chase_cases.py's
(its docstring says what they hold and tests/test_ref_chase_host.py that they reach every branch of the rule): eight codes from the perfect (7, 4)
to n = 256 and to 200 random 10-bit columns, patterns 0, 1, 3 and 6, w in {1, 4, 12}, the bit-packed map and the interleaver at depth 2 (ragged)
and C, K < n and K = n, both spreads, ties, a NaN, +-0 and +-inf, loud wrong bits around the used span.  Then runs of more codewords than a workgroup's tile, the grid-stride path (more tiles
of codewords than the launch has workgroups), two calls against each other, the stream pointers' absence, and the defaults of codewords and payload."""
import numpy as np
import pytest
import torch

import _chase_cases as K
import _ref_chase as X

pytestmark = pytest.mark.gpu

FIGS = ("status", "pre_err", "bit_err", "nflip", "erased", "pay_err")


def _run(case, llr, bits, **over):
    from vae_equalizer_amd.engine import HammingCode, chase_decode
    cols, r = K.CODES[case.code]
    kw = dict(t0=case.t0, codewords=case.C, depth=case.depth or None, patterns=case.p, payload=case.K, spread=bool(case.spread), want_stream=True)
    kw.update(over)
    ret = chase_decode(torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda(), HammingCode(cols, r), **kw)
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


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_chase_matches_model(case):
    llr, bits = K.tensors(case)
    _check(_run(case, llr, bits), K.expected(case), len(K.CODES[case.code][0]), case.K, case.name)


@pytest.mark.parametrize("case", K.TILES, ids=lambda c: c.name)
def test_several_tiles_per_run(case):
    llr, bits = K.tensors(case)
    _check(_run(case, llr, bits), K.expected(case), len(K.CODES[case.code][0]), case.K, case.name)


def test_grid_stride():
    case = K.STRIDE
    llr, bits = K.tensors(case)
    _check(_run(case, llr, bits), K.expected(case), len(K.CODES[case.code][0]), case.K, case.name)


@pytest.mark.parametrize("case", [K.CASES[i] for i in (7, 14, 23, 30)], ids=lambda c: c.name)
def test_repeatable_and_stream_optional(case):
    llr, bits = K.tensors(case)
    a, b, c = _run(case, llr, bits), _run(case, llr, bits), _run(case, llr, bits, want_stream=False)
    assert "stream" not in c and set(a) - set(c) == {"stream"}
    assert np.array_equal(_out(a), _out(b)) and np.array_equal(_out(a), _out(c))
    for k in ("llr", "bits"):
        assert torch.equal(a["stream"][k], b["stream"][k])
    for k in c:
        assert torch.equal(a[k], c[k]), k


def test_defaults():
    from vae_equalizer_amd.engine import HammingCode, chase_decode, hamming_code
    case = next(c for c in K.CASES if c.depth == 0 and c.w == 12)      # three spare symbols of 12 bits behind the C codewords
    cols, r = K.CODES[case.code]
    llr, bits = K.tensors(case)
    code = HammingCode(cols, r)
    fit = (llr.shape[-1] - case.t0) * case.w // code.n
    assert fit > case.C and code.k == code.n - r and (hamming_code(4, extended=False).k, hamming_code(5, n=20).k) == (11, 14)
    ret = chase_decode(torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda(), code, t0=case.t0, want_stream=True)
    want = X.decode(llr, bits, cols, 4, code.k, case.t0, fit, 0, 1)     # the defaults: every codeword that fits, patterns 4, payload k, spread
    _check(ret, want, code.n, code.k, "defaults")
    il = next(c for c in K.CASES if c.code == "e20" and c.depth)
    llr, bits = K.tensors(il)                                           # behind the interleaver the frame holds exactly C codewords
    ret = chase_decode(torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda(), hamming_code(5, n=20), t0=il.t0, depth=il.depth, patterns=il.p,
                       spread=bool(il.spread), want_stream=True)
    _check(ret, X.decode(llr, bits, K.CODES["e20"][0], il.p, 14, il.t0, il.C, il.depth, il.spread), 20, 14, "defaults-il")
