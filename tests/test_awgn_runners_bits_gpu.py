"""The AWGN host layer, pinned: what the three batch runners (run_awgn_batch, run_awgn_cma_batch, run_vaenn_batch), their ``processing`` wrappers,
the three sweep scripts' ``main()`` and the engine's result packers return must equal, array for array and bit for bit (dtype, shape, NaN
positions), what they returned when `tests/golden/G20_awgn_runners.npz` was recorded (tools/capture_awgn_runners.py, on an MI355X, with the Python
of the commit before the epoch loop, the sharded sweep and the result packing were each written once).  Every case is seeded, so the kernels see
the same inputs in the same order; a change of the host layer that keeps every launch, its arguments and the draw counter passes, and one that
reorders a draw, drops a launch or changes a float32 operation of NGMI does not.

Cases (each about a second):
  le/*      run_awgn_batch, 3 runs (nu 0 / 0.027 / 0.122), 64-QAM, M_est 25, both generators, want_info off and on; "hip" with 5 epochs at epe 2
            (the last epoch is not evaluated); "hip" at M_est 21, for which channel.awgn_clean_supported is false (the two-step validation)
  cma/*     run_awgn_cma_batch, 4 seeded runs (SNR 20 / 24), both generators; one unseeded run on the device generator
  nn/*      run_vaenn_batch, 2 runs, Net on "hip" and Net_BN on "numpy", want_info off and on
  proc/*    the three processing() wrappers, one run each
  main/*    the three scripts' main() on shrunk constants; every entry of save_dict
  pack/*    dp_epilogue, dp_epilogue_compact, cma_epilogue, dp_epilogue_info (q, y), awgn_info (q, y), cma_epilogue_info on planted launches of
            R = 3 runs of 400 symbols; every key of the returned dict
  print/*   one verbose single-run call of each runner; its standard output is part of the record
"""
import contextlib
import io
import tempfile

import numpy as np
import pytest
import torch

import _ref_awgn_info as A
import _ref_cma_info as C
import _ref_info as I
from conftest import load_golden

pytestmark = pytest.mark.gpu

FIXTURE = "G20_awgn_runners"
LE_RUNS = [dict(SNR=24, nu=nu, lr_optim=5e-3, seed=400 + i) for i, nu in enumerate((0.0, 0.0270955, 0.1222578))]
LE_ARGS = ("64-QAM", 2, 25, 100, 1200, 300, 4, 2, "h1")                  # mod, sps, M_est, batch_len, N_valid, N_train, num_epochs, epe, channel
CMA_RUNS = [dict(SNR=snr, nu=0.0, lr_optim=3e-4, seed=700 + 2 * j + k) for j, snr in enumerate((20, 24)) for k in range(2)]
CMA_ARGS = ("16-QAM", 2, 9, 3000, 2000, 6, 2, "h1")                      # mod, sps, M_est, N_valid, N_train, num_epochs, epe, channel
NN_RUNS = [dict(SNR=20, lr_optim=4e-3, seed=3), dict(SNR=24, lr_optim=4e-3, seed=1003)]
NN_ARGS = ("64-QAM", 2, 25, 25, 3, 300, 2000, 900, 4, 2, "h1")           # mod, sps, M_est, k1, k2, batch_len, N_valid, N_train, num_epochs, epe, channel
M_TWO_STEP = 21                                                          # odd, and not one of the tap counts the clean validation is built for


def _arrays(out, prefix=""):
    """A runner's return value -> {key: numpy array}: SER alone, or (SER, info)."""
    if isinstance(out, tuple):
        ser, info = out
        return {prefix + "SER": ser.numpy(), **{prefix + k: v.numpy() for k, v in info.items()}}
    return {prefix + "SER": out.numpy()}


def _le(generator, want_info, args=LE_ARGS, runs=LE_RUNS, **kw):
    from vae_equalizer_amd.func_VAELE_MQAM_shaping import run_awgn_batch
    return _arrays(run_awgn_batch(runs, *args, generator=generator, seed=11, want_info=want_info, **kw))


def _le_two_step():
    from vae_equalizer_amd import channel as ch
    assert not ch.awgn_clean_supported(2, M_TWO_STEP)
    return _le("hip", True, LE_ARGS[:2] + (M_TWO_STEP,) + LE_ARGS[3:])


def _cma(generator, runs=CMA_RUNS, **kw):
    from vae_equalizer_amd.func_CMA_MQAM_shaping import run_awgn_cma_batch
    return _arrays(run_awgn_cma_batch(runs, *CMA_ARGS, generator=generator, seed=7, **kw))


def _nn(net_type, generator, want_info, runs=NN_RUNS, **kw):
    from vae_equalizer_amd.func_VAENN_MQAM import run_vaenn_batch
    return _arrays(run_vaenn_batch(runs, *NN_ARGS, generator=generator, seed=5, net_type=net_type, want_info=want_info, **kw))


def _proc(which):
    from vae_equalizer_amd import func_CMA_MQAM_shaping as cma, func_VAELE_MQAM_shaping as le, func_VAENN_MQAM as nn
    if which == "le":
        return _arrays(le.processing("16-QAM", 2, 20, 0.0, 25, 5e-3, 100, 600, 300, 2, 2, "h1", seed=9, verbose=False, want_info=True))
    if which == "nn":
        return _arrays(nn.processing("16-QAM", 2, 20, 25, 25, 3, 4e-3, 100, 600, 300, 2, 2, "h1", "Net", seed=9, verbose=False, want_info=True))
    # the constant-modulus validation needs 1000 + 21 symbols
    return _arrays(cma.processing("16-QAM", 2, 20, 0.0, 9, 3e-4, 1200, 300, 2, 2, "h1", seed=9, verbose=False))


def _main(which, info_metrics=False):
    """The script's main() with the constants of its own test -> every entry of save_dict as an array."""
    import importlib
    ev = importlib.import_module("vae_equalizer_amd." + {"le": "Eval_run_shaping_vaele", "cma": "Eval_run_shaping_cma", "nn": "Eval_run_vaenn"}[which])
    const = {"le": dict(iter=2, num_epochs=4, N_valid=2000, base_seed=3, info_metrics=info_metrics),
             "nn": dict(iter=2, num_epochs=4, N_valid=2000, train_len=900, SNR_vec=[20, 24], base_seed=3, info_metrics=info_metrics),
             "cma": dict(mod="16-QAM", M_vec=[9, 25], lr_optim_vec=[3e-4], SNR_vec=[20, 24], iter=2, N_valid=3000, train_len=2000, num_epochs=6,
                         base_seed=11)}[which]
    with tempfile.TemporaryDirectory() as tmp, pytest.MonkeyPatch.context() as mp:
        for k, v in dict(const, savePATH=tmp + "/").items():
            mp.setattr(ev, k, v)
        _, d = ev.main()
    return {k: np.asarray(v) for k, v in d.items()}


def _stack(xs, *keys):
    return {k: torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(x[k]) for x in xs]))).cuda() for k in keys}


def _pack(which):
    """One call of an engine wrapper on a planted launch of R = 3 runs, N = 400 -> every key of the dict it returns."""
    from vae_equalizer_amd import engine
    if which.startswith("awgn_info"):
        xs = _awgn_400()
        src = _stack(xs, "q") if which.endswith("q") else _stack(xs, "y", "amp_mean", "var")
        out = engine.awgn_info(data=_stack(xs, "tx")["tx"], amp_levels=xs[0]["amp"], **_stack(xs, "P", "shift"), **src)
    elif which.startswith("cma"):
        xs = C.build_launch("N400-n4")[0]
        base = dict(data=_stack(xs, "tx")["tx"], amp_levels=xs[0]["amp"], **_stack(xs, "y", "nu_sc", "var"))
        out = (engine.cma_epilogue(**base) if which == "cma_epilogue" else
               engine.cma_epilogue_info(**base, **_stack(xs, "P", "shift_c", "r_c", "shift_q", "r_q")))
    else:
        xs = I.build_launch("N400-B20-n4")[0]
        base = dict(data=_stack(xs, "tx")["tx"], amp_levels=xs[0]["amp"], batch_len=xs[0]["batch_len"])
        if which == "dp_epilogue":
            out = engine.dp_epilogue(**base, **_stack(xs, "q", "y", "nu_sc", "var"))
        elif which == "dp_epilogue_compact":
            n = xs[0]["n"]
            q = np.stack([x["q"] for x in xs])                                  # [R,2,2n,N]
            eq = (q[:, :, :n] * xs[0]["amp"][None, None, :, None]).sum(2, dtype=np.float32)
            dec = np.stack([q[:, :, :n].argmax(2), q[:, :, n:].argmax(2)], 2).astype(np.int8)
            out = engine.dp_epilogue_compact(torch.from_numpy(eq).cuda(), torch.from_numpy(dec).cuda(), **base, **_stack(xs, "y", "nu_sc", "var"))
        else:
            src = _stack(xs, "q") if which.endswith("q") else _stack(xs, "y", "nu_sc", "var")
            out = engine.dp_epilogue_info(**base, **_stack(xs, "P", "shift", "r"), **src)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _awgn_400():
    """_ref_awgn_info has no launch of 400 symbols: three of its planted runs at N = 400 (n_lev 4; shifts of both signs, three hypotheses)."""
    return [A.make_run(seed=20000 + k, N=400, n=4, shift=sh, hyp=k + 1, nu=nu, var=A.VARS[k], n_err=3)
            for k, (sh, nu) in enumerate(((-7, 0.0), (0, 0.05), (9, 0.1)))]


def _printed(fn):
    """fn() with its standard output recorded beside its arrays."""
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = fn()
    return dict(out, stdout=np.array(buf.getvalue()))


CASES = {
    "le/hip/ser": lambda: _le("hip", False), "le/hip/info": lambda: _le("hip", True),
    "le/numpy/ser": lambda: _le("numpy", False), "le/numpy/info": lambda: _le("numpy", True),
    "le/hip/5-epochs": lambda: _le("hip", True, LE_ARGS[:6] + (5, 2, "h1")),
    "le/hip/two-step": _le_two_step,
    "cma/hip": lambda: _cma("hip"), "cma/numpy": lambda: _cma("numpy"),
    "cma/hip/unseeded-single": lambda: _cma("hip", [dict(SNR=22, nu=0.0, lr_optim=3e-4, seed=None)]),
    "nn/Net/hip/ser": lambda: _nn("Net", "hip", False), "nn/Net/hip/info": lambda: _nn("Net", "hip", True),
    "nn/Net_BN/numpy/ser": lambda: _nn("Net_BN", "numpy", False), "nn/Net_BN/numpy/info": lambda: _nn("Net_BN", "numpy", True),
    "proc/le": lambda: _proc("le"), "proc/cma": lambda: _proc("cma"), "proc/nn": lambda: _proc("nn"),
    "main/le/ser": lambda: _main("le"), "main/le/info": lambda: _main("le", True),
    "main/nn/ser": lambda: _main("nn"), "main/nn/info": lambda: _main("nn", True), "main/cma": lambda: _main("cma"),
    **{"pack/" + w: (lambda w=w: _pack(w)) for w in ("dp_epilogue", "dp_epilogue_compact", "cma_epilogue", "dp_epilogue_info/q", "dp_epilogue_info/y",
                                                   "awgn_info/q", "awgn_info/y", "cma_epilogue_info")},
    "print/le": lambda: _printed(lambda: _le("hip", True, runs=LE_RUNS[1:2], verbose=True)),
    "print/cma": lambda: _printed(lambda: _cma("hip", CMA_RUNS[:1], verbose=True)),
    "print/nn": lambda: _printed(lambda: _nn("Net", "hip", True, runs=NN_RUNS[:1], verbose=True)),
}


def same_bits(a, b):
    """dtype, shape and every byte, so that NaN equals NaN only at the same place and with the same bits."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.fixture(scope="module")
def recorded():
    return load_golden(FIXTURE)


def test_the_fixture_holds_exactly_these_cases(recorded):
    assert {k.split("//")[0] for k in recorded} == set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_awgn_runner_bits(name, recorded):
    got = CASES[name]()
    want = {k.split("//")[1]: v for k, v in recorded.items() if k.split("//")[0] == name}
    assert set(got) == set(want)
    for k in got:
        assert same_bits(got[k], want[k]), "%s: got %s %s, recorded %s %s" % (k, np.asarray(got[k]).dtype, np.asarray(got[k]).tolist(), want[k].dtype,
                                                                            want[k].tolist())
    if name.startswith("print/"):
        assert str(want["stdout"]).count("SER = ") >= 2                         # the recorded text has a line per evaluated epoch
