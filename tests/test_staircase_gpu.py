"""vaeq_staircase_decode on the device against its integer model (tests/_ref_staircase.py), with no tolerance: np.array_equal on out, hard,
pos_err and pos_iters.  The cases are tests/_staircase_cases.py's -- seven component codes (a perfect code; rows far below a word and s below a
wave, twice; one bit under a word; a row that crosses a word with 2 s > 64; more than one wave of components, ragged; word-aligned), each with
one pair, one position, a window of two with one iteration, the cap and L = W, at 0.3, 1 and 2 times t / (2 s) errors per bit, chains that start
inside a symbol, loud wrong bits all around them and a NaN, a +0 and a -0 inside.  Before the device is asked, the model's counters say that
every branch of the rule was taken (tests/test_ref_staircase_host.py asserts the same without a device).

Then: the four values of t the shapes leave out, the largest state within 64 KiB, two calls agreeing bit for bit, optional outputs changing nothing, and the t0 / chains defaults."""
import collections

import numpy as np
import pytest
import torch

import _ref_staircase as S
import _staircase_cases as K

pytestmark = pytest.mark.gpu

FIGS = ("iters", "ok", "bit_err", "pre_err", "erased", "iters_max", "nflip", "bad_flips")


def _code(m, t, s, L):
    from vae_equalizer_amd.engine import BchCode, StaircaseCode
    return StaircaseCode(BchCode(m, t, n=2 * s), L)


def _decode(c, **kw):
    from vae_equalizer_amd.engine import staircase_decode
    kw = dict(dict(t0=c["t0"], chains=K.C_, iters=c["iters"], want_hard=True, want_profile=True), **kw)
    return staircase_decode(torch.from_numpy(c["llr"].copy()).cuda(), torch.from_numpy(c["bits"].copy()).cuda(), _code(c["m"], c["t"], c["s"], c["L"]),
                            c["W"], **kw)


def _same(got, c, tag):
    out = np.stack([got[k].cpu().numpy() for k in FIGS], -1)
    diff = {k: int((a != b).sum()) for k, a, b in (("out", out, c["out"]), ("hard", got["hard"].cpu().numpy(), c["hard"]),
                                                   ("pos_err", got["pos_err"].cpu().numpy(), c["pos_err"]),
                                                   ("pos_iters", got["pos_iters"].cpu().numpy(), c["pos_iters"]))}
    print(f"{tag}: pre_err {c['out'][..., 3].ravel().tolist()} post_err {c['out'][..., 2].ravel().tolist()} iters {c['out'][..., 0].ravel().tolist()} "
          f"nflip {c['out'][..., 6].ravel().tolist()} bad_flips {c['out'][..., 7].ravel().tolist()}; the kernel differs in {diff}")
    assert not any(diff.values()), (tag, diff)
    assert got["positions"] == S.n_positions(c["L"], c["W"]) and got["hard"].dtype == torch.int8


@pytest.mark.parametrize("a", range(len(K.LWI)), ids=lambda a: "L%d-W%d-it%d" % K.LWI[a])
@pytest.mark.parametrize("shape", K.SHAPES, ids=str)
def test_kernel_equals_model(shape, a):
    count = K.counts(shape)
    assert all(count[k] > 0 for k in K.reached(shape)), [k for k in K.reached(shape) if not count[k]]
    for b in range(len(K.RATES)):
        c = K.case(shape, a, b)
        _same(_decode(c), c, f"{shape} L={c['L']} W={c['W']} iters={c['iters']} rate x{K.RATES[b]} w={c['w']} t0={c['t0']}")


@pytest.mark.parametrize("t", (4, 5, 6, 7))
def test_every_correction_capability(t):
    """The kernel is compiled once per t: the shapes above run t = 1, 2 and 3 and the largest state t = 8; these are the four between, over
    GF(2^7) with s = 40 (rows that cross a word, 2 s > 64), at 1 and 1.6 times t / (2 s) so that L = t, L > t and roots < L all occur."""
    m, s, L, W, iters, w, t0 = 7, 40, 3, 2, 3, 12, 11
    for rate in (1.0, 1.6):
        llr, bits = K.make(900 + t, m, t, s, L, rate, w, t0)
        count = collections.Counter()
        out, hard, pos_err, pos_iters, _ = S.decode(llr, bits, m, t, s, L, W, iters, t0, K.C_, count)
        assert count["status1"] > 0 and (rate == 1.0 or (count["L>t"] > 0 and count["roots<L"] > 0)), dict(count)
        c = dict(m=m, t=t, s=s, L=L, W=W, iters=iters, w=w, t0=t0, llr=llr, bits=bits, out=out, hard=hard, pos_err=pos_err, pos_iters=pos_iters)
        _same(_decode(c), c, f"t = {t}, rate x{rate}")


def test_largest_state():
    """(m, t, s) = (10, 8, 349) with a window of one pair: 65 520 bytes of the 65 536 (tests/test_abi_refusals_staircase_host.py has the refusal
    one step above), 384 threads of which 349 work, rows of 11 words."""
    from vae_equalizer_amd import _native as nat
    m, t, s, L, W, iters, w, t0 = 10, 8, 349, 2, 1, 3, 12, 5
    assert nat.lib().vaeq_staircase_lds_bytes(m, s, W) == 65520
    llr, bits = K.make(77, m, t, s, L, 1.2, w, t0)
    llr, bits = llr[:1], bits[:1]
    count = collections.Counter()
    out, hard, pos_err, pos_iters, _ = S.decode(llr, bits, m, t, s, L, W, iters, t0, K.C_, count)
    assert count["status1"] > 0 and count["status2"] > 0 and out[..., 6].min() > 0 and out[..., 2].min() > 0
    c = dict(m=m, t=t, s=s, L=L, W=W, iters=iters, w=w, t0=t0, llr=llr, bits=bits, out=out, hard=hard, pos_err=pos_err, pos_iters=pos_iters)
    _same(_decode(c), c, "largest state")


def test_two_calls_agree_and_optional_outputs_change_nothing():
    c = K.case((7, 2, 33), 3, 1)
    a, b = _decode(c), _decode(c)
    plain = _decode(c, want_hard=False, want_profile=False)
    hard_only = _decode(c, want_profile=False)
    assert set(a) == set(b) == set(plain) | {"hard", "pos_err", "pos_iters"} and set(hard_only) == set(plain) | {"hard"}
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k
    for k in plain:
        assert torch.equal(a[k], plain[k]) and torch.equal(a[k], hard_only[k]) if torch.is_tensor(a[k]) else a[k] == plain[k] == hard_only[k], k
    assert torch.equal(a["hard"], hard_only["hard"])
    for k in ("BER_post", "BER_pre", "FER"):
        assert a[k].dtype == torch.float32 and tuple(a[k].shape) == (K.R_,)
    n = c["L"] * c["s"] ** 2
    assert np.array_equal(a["BER_post"].cpu().numpy(), (c["out"][..., 2].sum(1) / np.float32(K.C_ * n)).astype(np.float32))
    assert np.array_equal(a["BER_pre"].cpu().numpy(), (c["out"][..., 3].sum(1) / np.float32(K.C_ * n)).astype(np.float32))
    assert np.array_equal(a["FER"].cpu().numpy(), (c["out"][..., 2] > 0).mean(1).astype(np.float32))


def test_defaults_of_t0_and_chains():
    """t0 = 0 and the most chains that fit: a frame of the case's tensors cut to start at the first chain and to hold one chain more."""
    from vae_equalizer_amd.engine import staircase_decode
    shape, (m, t, s) = (5, 2, 15), (5, 2, 15)
    L, W, iters, w = 4, 2, 3, 8
    llr, bits = K.make(5, m, t, s, L, 1.0, w, 0)            # N = ceil(2 n / 8) + 3 = 228 symbols: 1824 bits, two chains of 900 and no third
    assert llr.shape[-1] * w // (L * s * s) == 2
    out, hard, pos_err, pos_iters, _ = S.decode(llr, bits, m, t, s, L, W, iters, 0, 2)
    got = staircase_decode(torch.from_numpy(llr).cuda(), torch.from_numpy(bits).cuda(), _code(m, t, s, L), W, iters=iters, want_hard=True,
                           want_profile=True)
    c = dict(L=L, W=W, out=out, hard=hard, pos_err=pos_err, pos_iters=pos_iters)
    _same(got, c, f"defaults {shape}")
    with pytest.raises(ValueError):
        staircase_decode(torch.from_numpy(llr[..., :100]).cuda(), torch.from_numpy(bits[..., :100]).cuda(), _code(m, t, s, L), W)
    four = staircase_decode(torch.from_numpy(llr.reshape(K.R_, 2, 4, -1)).cuda(), torch.from_numpy(bits.reshape(K.R_, 2, 4, -1)).cuda(), _code(m, t, s, L),
                            W, iters=iters)                 # the DP tensors [R, 2, 2b, N]
    assert all(torch.equal(four[k], got[k]) for k in FIGS)
