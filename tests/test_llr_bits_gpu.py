"""The bits of the four LLR kernels and of vaeq_awgn_track_info, pinned: every row of LLR planes and the seven arrays of every track launch must
equal, bit for bit, what the kernels computed when `tests/golden/G22_llr_bits.npz` was recorded (tools/capture_llr_bits.py, on an MI355X, with
the library of the commit before each information-rate kernel and its LLR sibling were put on one window, one pre-pass and one demapper).  The
float64 models of the LLR tests allow several float32 deviations; a change that only moves text has to leave summation order, operands and
roundings alone, so it passes here and nothing else does.  tests/test_info_bits_gpu.py does the same for the other three information-rate kernels.

An LLR launch is recorded as one sha256 per (run, polarisation) over the float32 bytes of that row of planes [2 b, N]: a few kilobytes for the
whole fixture, and a -0.0 where an erasure, +0.0, belongs is another digest.  The hypotheses an LLR launch takes are recorded figures (G19 for the
DP, AWGN and CMA kernels, this fixture's track part for the track kernel), so no LLR case depends on an information-rate launch of the build under
test.

Launches: test_info_bits_gpu.py's for dp, awgn and cma (every one of _ref_info.LAUNCHES and _ref_awgn_info.LAUNCHES in q- and y-mode, of
_ref_cma_info.LAUNCHES, and the launch "K0" of each); for the track pair every one of _ref_awgn_baseline_info.LAUNCHES, "wide" (two calls:
Nz = Nd + 1 for its first run, Nz = Nd for the other two) and two launches of D38-e31-dz1-il1-n4 whose middle run keeps nothing:
  K0-zero   z[1] = 0: no mean radius, no normalisation
  K0-empty  shift[1] = -edge: an empty window
A run that keeps nothing is a row of +0.0 (LLR) or NaN figures with zero counts (track info), between two runs that keep their symbols.
"""
import functools
import hashlib

import numpy as np
import pytest
import torch

import _ref_awgn_baseline_info as T
import test_info_bits_gpu as G
from conftest import load_golden

pytestmark = pytest.mark.gpu

FIXTURE = "G22_llr_bits"
K0_TRACK = ("K0-zero", "K0-empty")
KEYS = G.KEYS
TRACK_INPUTS = ("z", "tx", "amp", "P", "var", "shift", "edge", "interleaved")
CASES = G.CASES + [("track", "y", n) for n in T.LAUNCHES + ["wide"] + list(K0_TRACK)]


@functools.lru_cache(maxsize=None)
def build_inputs(kernel, name):
    """The per-run inputs of a launch, rebuilt from its seeds."""
    if kernel != "track":
        return G.build_inputs(kernel, name)
    if name not in K0_TRACK:
        return T.build_launch(name)[0]
    xs = T.build_launch("D38-e31-dz1-il1-n4")[0]
    return [xs[0], dict(xs[1], z=np.zeros_like(xs[1]["z"])) if name == "K0-zero" else dict(xs[1], shift=-xs[1]["edge"]), xs[2]]


def digest(kernel, xs):
    if kernel != "track":
        return G.digest(kernel, xs)
    h = hashlib.sha256()
    for x in xs:
        for k in TRACK_INPUTS:
            a = np.asarray(x[k])
            h.update(("%s %s %s " % (k, a.dtype.str, a.shape)).encode() + np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _dev(xs, *keys):
    return {k: torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(x[k]) for x in xs]))).cuda() for k in keys}


def _track_calls(xs):
    """The engine calls of a track launch: one, or one per length of z ("wide") -> [(runs, keyword arguments both track functions take)]."""
    out = []
    for dz in sorted({x["z"].shape[-1] - x["tx"].shape[-1] for x in xs}, reverse=True):
        idx = [i for i, x in enumerate(xs) if x["z"].shape[-1] - x["tx"].shape[-1] == dz]
        sub = [xs[i] for i in idx]
        z = _dev(sub, "z")["z"]
        z = z if sub[0]["interleaved"] else torch.stack([z.real, z.imag], 1).contiguous()
        out.append((idx, dict(z=z, data=_dev(sub, "tx")["tx"], amp_levels=sub[0]["amp"], edge=sub[0]["edge"], **_dev(sub, "var", "shift"))))
    return out


def run_track_info(xs):
    """engine.awgn_track_info on cuda:0 -> {key: numpy array [R]}, float32 figures and int64 counts as the engine returns them."""
    from vae_equalizer_amd import engine
    got = {k: [None] * len(xs) for k in KEYS}
    for idx, kw in _track_calls(xs):
        out = engine.awgn_track_info(P=_dev([xs[i] for i in idx], "P")["P"], **kw)
        for k in KEYS:
            for i, v in zip(idx, out[k].cpu().numpy()):
                got[k][i] = v
    return {k: np.stack(v) for k, v in got.items()}


def run_llr(kernel, mode, xs, hyp):
    """One call of the engine's LLR function on cuda:0 under the hypotheses hyp -> llr[R, (2,) 2 b, N] float32 as a numpy array."""
    from vae_equalizer_amd import engine
    kw = dict(amp_levels=xs[0]["amp"], hyp=torch.from_numpy(np.ascontiguousarray(hyp)).cuda())
    if kernel == "dp":
        out = engine.dp_epilogue_llr(batch_len=xs[0]["batch_len"], **_dev(xs, "shift", "r"),
                                     **(_dev(xs, "q") if mode == "q" else _dev(xs, "y", "nu_sc", "var")), **kw)
    elif kernel == "awgn":
        out = engine.awgn_llr(**_dev(xs, "shift"), **(_dev(xs, "q") if mode == "q" else _dev(xs, "y", "amp_mean", "var")), **kw)
    elif kernel == "cma":
        out = engine.cma_epilogue_llr(data=_dev(xs, "tx")["tx"], **_dev(xs, "y", "nu_sc", "var", "shift_c", "r_c", "shift_q", "r_q"), **kw)
    else:
        rows = [None] * len(xs)
        for idx, tkw in _track_calls(xs):
            res = engine.awgn_track_llr(**dict(tkw, amp_levels=kw["amp_levels"], hyp=kw["hyp"][idx])).cpu().numpy()
            for i, v in zip(idx, res):
                rows[i] = v
        return np.stack(rows)
    return out.cpu().numpy()


def row_digests(llr):
    """llr[R, 2, 2 b, N] or [R, 2 b, N] float32 -> the sha256 of every row of planes, an array of str [R, 2] or [R]."""
    assert llr.dtype == np.float32 and llr.ndim in (3, 4)
    flat = np.ascontiguousarray(llr).reshape(-1, llr.shape[-2] * llr.shape[-1])
    return np.array([hashlib.sha256(r.tobytes()).hexdigest() for r in flat]).reshape(llr.shape[:-2])


def zero_digest(llr):
    return hashlib.sha256(np.zeros(llr.shape[-2] * llr.shape[-1], np.float32).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def recorded():
    return load_golden(FIXTURE)


@pytest.fixture(scope="module")
def figures():
    return load_golden(G.FIXTURE)


def recorded_figures(kernel, mode, name, recorded, figures):
    """(kept, hyp) of a launch as recorded: the track kernel's in this fixture, the others' in test_info_bits_gpu.py's."""
    src = recorded if kernel == "track" else figures
    return tuple(src["%s/%s/%s/%s" % (kernel, mode, name, k)] for k in ("kept", "hyp"))


def test_the_fixture_holds_exactly_these_cases(recorded):
    want = {"%s/%s/%s/llr" % c for c in CASES} | {"%s/%s/sha256" % (k, n) for k, _, n in CASES}
    want |= {"%s/%s/%s/%s" % (c + (k,)) for c in CASES if c[0] == "track" for k in KEYS}
    assert set(recorded) == want


@pytest.mark.parametrize("name", [c[2] for c in CASES if c[0] == "track"])
def test_track_info_bits(name, recorded):
    xs = build_inputs("track", name)
    assert digest("track", xs) == str(recorded["track/%s/sha256" % name]), "the seeded input is not the one the fixture was recorded with"
    got = run_track_info(xs)
    want = {k: recorded["track/y/%s/%s" % (name, k)] for k in KEYS}
    for k in KEYS:
        assert got[k].dtype == (np.int64 if k in KEYS[3:] else np.float32) and got[k].shape == (3,), k
        assert G.same_bits(got[k], want[k]), "%s: got %s, recorded %s" % (k, got[k].tolist(), want[k].tolist())
    if name in K0_TRACK:                                                       # the recorded launch is the one described above
        assert (want["kept"] == 0).tolist() == [False, True, False]
        assert all(np.isnan(want[k][1]) and np.isfinite(want[k][[0, 2]]).all() for k in KEYS[:3])
        assert all(want[k][1] == 0 for k in KEYS[3:])


@pytest.mark.parametrize("kernel,mode,name", CASES, ids=["-".join(c) for c in CASES])
def test_llr_bits(kernel, mode, name, recorded, figures):
    xs = build_inputs(kernel, name)
    assert digest(kernel, xs) == str(recorded["%s/%s/sha256" % (kernel, name)]), "the seeded input is not the one the fixture was recorded with"
    kept, hyp = recorded_figures(kernel, mode, name, recorded, figures)
    llr = run_llr(kernel, mode, xs, hyp)
    got, want = row_digests(llr), recorded["%s/%s/%s/llr" % (kernel, mode, name)]
    assert got.shape == want.shape == kept.shape == ((3, 2) if kernel in ("dp", "cma") else (3,))
    differ = np.argwhere(got != want).tolist()
    assert not differ, "the rows (run, polarisation) %s are not the recorded bits" % differ
    assert ((want == zero_digest(llr)) == (kept == 0)).all(), "exactly the rows that keep nothing are all +0.0"
    if name == G.K0 or name in K0_TRACK:                                       # the recorded launch is the one described above
        assert (kept == 0).reshape(3, -1).all(axis=1).sum() == 1
