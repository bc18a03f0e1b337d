"""The bits of the three information-rate kernels, pinned: AIR, GMI, BER and the four counts of every launch must equal, array for array and bit
for bit, what the kernels computed when `tests/golden/G19_info_bits.npz` was recorded (tools/capture_info_bits.py, on an MI355X, with the library
of the commit before the three kernels were put on one per-symbol body and one tail).  The float64 models of tests/test_epilogue_info_gpu.py,
test_awgn_info_gpu.py and test_cma_info_gpu.py allow three times the float32 deviation; a change that only moves text has to leave summation
order, operands and roundings alone, so it passes here and nothing else does.

Launches: every one of _ref_info.LAUNCHES and _ref_awgn_info.LAUNCHES in q- and y-mode and of _ref_cma_info.LAUNCHES (R = 3 runs each: every
template instance, hypothesis and shift sign, partial and multiple strides of 256 threads), and per kernel one launch "K0" in which one run
keeps nothing (NaN figures, zero counts) between two that do:
  dp    N43-B0-n2 evaluated with batch_len = 43: the per-minibatch cut leaves 11 / 1 / 0 symbols
  awgn  N = 22, n_lev = 2, shifts -10 / -5 / 0: 10 / 5 / 0 symbols
  cma   N400-n8 with y[1] = 0: no mean radius, no normalisation
NGMI is formed on the host from GMI and is not recorded.
"""
import functools
import hashlib

import numpy as np
import pytest
import torch

import _ref_awgn_info as A
import _ref_cma_info as C
import _ref_info as I
from conftest import load_golden

pytestmark = pytest.mark.gpu

FIXTURE = "G19_info_bits"
K0 = "K0"
KEYS = ("AIR", "GMI", "BER", "kept", "sym_err", "bit_err", "hyp")
INPUTS = {"dp": ("q", "y", "tx", "amp", "P", "nu_sc", "var", "shift", "r", "batch_len"),
          "awgn": ("q", "y", "tx", "amp", "P", "amp_mean", "var", "shift"),
          "cma": ("y", "tx", "amp", "P", "nu_sc", "var", "shift_c", "r_c", "shift_q", "r_q")}
CASES = ([("dp", m, n) for n in I.LAUNCHES + [K0] for m in "qy"] + [("awgn", m, n) for n in A.LAUNCHES + [K0] for m in "qy"]
         + [("cma", "y", n) for n in C.LAUNCHES + [K0]])


@functools.lru_cache(maxsize=None)
def build_inputs(kernel, name):
    """The per-run inputs of a launch, rebuilt from its seeds."""
    if kernel == "dp":
        return [dict(x, batch_len=43) for x in I.build_launch("N43-B0-n2")[0]] if name == K0 else I.build_launch(name)[0]
    if kernel == "awgn":
        if name == K0:
            return [A.make_run(seed=19000 + k, N=22, n=2, shift=sh, hyp=k, nu=0.0, var=A.VARS[k], n_err=1) for k, sh in enumerate((-10, -5, 0))]
        return A.build_launch(name)[0]
    xs = C.build_launch("N400-n8" if name == K0 else name)[0]
    return [xs[0], dict(xs[1], y=np.zeros_like(xs[1]["y"])), xs[2]] if name == K0 else xs


def digest(kernel, xs):
    h = hashlib.sha256()
    for x in xs:
        for k in INPUTS[kernel]:
            v = x[k]
            a = np.asarray(0 if v is None else v)
            h.update(("%s %s %s " % (k, a.dtype.str, a.shape)).encode() + np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_launch(kernel, mode, xs):
    """One call of the engine function on cuda:0 -> {key: numpy array}, float32 figures and int64 counts as the engine returns them."""
    from vae_equalizer_amd import engine

    def d(*keys):
        return {k: torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(x[k]) for x in xs]))).cuda() for k in keys}
    kw = dict(data=d("tx")["tx"], amp_levels=xs[0]["amp"], **d("P"))
    if kernel == "dp":
        out = engine.dp_epilogue_info(shift=d("shift")["shift"], r=d("r")["r"], batch_len=xs[0]["batch_len"],
                                      **(d("q") if mode == "q" else d("y", "nu_sc", "var")), **kw)
    elif kernel == "awgn":
        out = engine.awgn_info(**d("shift"), **(d("q") if mode == "q" else d("y", "amp_mean", "var")), **kw)
    else:
        out = engine.cma_epilogue_info(**d("y", "nu_sc", "var", "shift_c", "r_c", "shift_q", "r_q"), **kw)
    return {k: out[k].cpu().numpy() for k in KEYS}


def same_bits(a, b):
    """dtype, shape and every bit; floats through their uint32 view, so that NaN equals NaN."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = (lambda v: v.view(np.uint32)) if a.dtype == np.float32 else (lambda v: v)
    return np.array_equal(view(np.ascontiguousarray(a)), view(np.ascontiguousarray(b)))


@pytest.fixture(scope="module")
def recorded():
    return load_golden(FIXTURE)


def test_the_fixture_holds_exactly_these_cases(recorded):
    want = {"%s/%s/%s/%s" % (c + (k,)) for c in CASES for k in KEYS} | {"%s/%s/sha256" % (k, n) for k, _, n in CASES}
    assert set(recorded) == want


@pytest.mark.parametrize("kernel,mode,name", CASES, ids=["-".join(c) for c in CASES])
def test_info_bits(kernel, mode, name, recorded):
    xs = build_inputs(kernel, name)
    assert digest(kernel, xs) == str(recorded["%s/%s/sha256" % (kernel, name)]), "the seeded input is not the one the fixture was recorded with"
    got = run_launch(kernel, mode, xs)
    want = {k: recorded["%s/%s/%s/%s" % (kernel, mode, name, k)] for k in KEYS}
    shape = (3,) if kernel == "awgn" else (3, 2)
    for k in KEYS:
        assert got[k].dtype == (np.int64 if k in KEYS[3:] else np.float32) and got[k].shape == shape, k
        assert same_bits(got[k], want[k]), "%s: got %s, recorded %s" % (k, got[k].tolist(), want[k].tolist())
    empty = (want["kept"] == 0).reshape(3, -1).all(axis=1)
    if name == K0:                                                             # the recorded launch is the one described above
        assert empty.sum() == 1 and all(np.isnan(want[k].reshape(3, -1)[empty]).all() for k in KEYS[:3])
        assert all(np.isfinite(want[k].reshape(3, -1)[~empty]).all() for k in KEYS[:3])
