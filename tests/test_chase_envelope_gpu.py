"""vaeq_chase_decode over the parts of include/vaeq.h's envelope that tests/test_chase_gpu.py leaves out, through engine.chase_decode against
the model of tests/_ref_chase.py, bit for bit: out[R, C, 6] and both tensors of the payload stream with np.array_equal, no tolerance.  The cases
live in tests/_chase_envelope_cases.py (its docstring lists them); tests/test_ref_fec_envelope_host.py asserts on the CPU that the model reaches
in them what this file relies on.  Every test prints its figures before it asserts.

  the smallest codes (n = 3 with p = n, n = 4), words of one, two, three and four lane slots at their boundaries, ten-bit columns with both ends
  of the syndrome table, every tile size with two full tiles and a ragged one under both maps and both spreads, w in {2, 3, 5, 7, 13, 64},
  K = 1 and K = n - 1, 40 runs of one codeword and a tile of one word, and whole codewords of zeros and NaN, of infinities and of one magnitude."""
import numpy as np
import pytest
import torch

import _chase_envelope_cases as E
import _ref_chase as X

pytestmark = pytest.mark.gpu

FIGS = ("status", "pre_err", "bit_err", "nflip", "erased", "pay_err")


def _run(case, llr, bits):
    from vae_equalizer_amd.engine import HammingCode, chase_decode
    cols, r = E.CODES[case.code]
    ret = chase_decode(torch.from_numpy(llr.copy()).cuda(), torch.from_numpy(bits.copy()).cuda(), HammingCode(cols, r), t0=case.t0, codewords=case.C,
                       depth=case.depth or None, patterns=case.p, payload=case.K, spread=bool(case.spread), want_stream=True)
    torch.cuda.synchronize()
    return ret


def _check(ret, want, n, Kp, tag):
    out, s_llr, s_bits, _ = want
    got = np.stack([ret[k].cpu().numpy() for k in FIGS], -1)
    g_llr, g_bits = ret["stream"]["llr"].cpu().numpy(), ret["stream"]["bits"].cpu().numpy()
    print(f"{tag}: status {np.bincount(out[..., 0].ravel(), minlength=3).tolist()} pre_err {int(out[..., 1].sum())} post_err {int(out[..., 2].sum())} "
          f"flips {int(out[..., 3].sum())} erased {int(out[..., 4].sum())} pay_err {int(out[..., 5].sum())}; out differs in {int((got != out).sum())}, "
          f"stream llr in {int((g_llr[:, 0] != s_llr).sum())}, stream bits in {int((g_bits[:, 0] != s_bits).sum())} of {s_bits.size}")
    assert got.dtype == np.int64 and g_llr.dtype == np.float32 and g_bits.dtype == np.int8
    assert g_llr.shape == (out.shape[0], 1, s_llr.shape[1]) and g_bits.shape == g_llr.shape
    assert np.array_equal(got, out)
    assert np.array_equal(g_llr[:, 0].view(np.uint32), s_llr.view(np.uint32)) and np.array_equal(g_bits[:, 0], s_bits)
    for k, v in X.figures(out, n, Kp).items():
        assert np.array_equal(ret[k].cpu().numpy(), v), k


@pytest.mark.parametrize("case", [c for g in ("smallest", "slots", "top", "widths", "payload", "grid") for c in E.GROUPS[g]], ids=lambda c: c.name)
def test_chase_matches_model(case):
    llr, bits = E.tensors(case)
    _check(_run(case, llr, bits), E.expected(case), E.n_of(case), case.K, case.name)


@pytest.mark.parametrize("case", E.GROUPS["tiles"], ids=lambda c: c.name)
def test_every_tile_size(case):
    tw = E.TILE_WORDS[E.n_of(case)]
    assert 2 * tw < case.C < 3 * tw and case.K < E.n_of(case) and (not case.depth or tw % case.depth)
    llr, bits = E.tensors(case)
    _check(_run(case, llr, bits), E.expected(case), E.n_of(case), case.K, case.name)


@pytest.mark.parametrize("case", E.DEGENERATE, ids=lambda c: c.name)
def test_degenerate_reliabilities(case):
    llr, bits = E.tensors(case, True)
    want = E.expected(case, True)
    assert (want[0][:, E.ZEROS, 4] == E.n_of(case)).all() and not want[0][:, E.INFS, 4].any()
    _check(_run(case, llr, bits), want, E.n_of(case), case.K, case.name)
