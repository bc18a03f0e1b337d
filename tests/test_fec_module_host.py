"""vae_equalizer_amd/fec.py, the FEC host layer: the names engine.py re-exports, the shape of the fec= dispatch table and the one division behind
every rate figure.  No GPU."""
import numpy as np
import pytest
import torch

PUBLIC = ("label_bits", "LdpcCode", "array_code", "ScLdpcCode", "sc_array_code", "BchCode", "StaircaseCode", "HammingCode", "hamming_code", "EbchCode",
          "ebch_code", "ProductCode", "resolve_quant", "resolve_outer", "resolve_inner", "resolve_tpc", "ldpc_decode", "ldpc_sc_decode", "bch_outer",
          "staircase_decode", "chase_decode", "tpc_decode", "check_fec", "fec_figures", "QUANT_KEYS", "OUTER_KEYS", "OUTER_POST_BYTES", "INNER_KEYS",
          "FEC_KEYS", "FEC_BLOCK_ONLY", "FEC_SC_ONLY", "FEC_STAIRCASE_KEYS", "FEC_TPC_KEYS", "TPC_ALPHA", "TPC_BETA", "TPC_CLIP")


def test_engine_exposes_the_objects_of_fec():
    from vae_equalizer_amd import engine, fec
    assert len(set(PUBLIC)) == 36
    for name in PUBLIC:
        assert getattr(engine, name) is getattr(fec, name), name
    public = {k for k, v in vars(fec).items() if not k.startswith("_") and getattr(v, "__module__", fec.__name__) == fec.__name__
              and not isinstance(v, type(fec))}
    assert public == set(PUBLIC)                             # a new public name of fec.py is a decision about engine's list too
    assert not [k for k in vars(engine) if k.startswith("_") and not k.startswith("__") and hasattr(fec, k)]   # and no private name crosses


def test_one_row_per_code_class():
    from vae_equalizer_amd import fec
    from vae_equalizer_amd.fec import (BchCode, LdpcCode, ProductCode, ScLdpcCode, StaircaseCode, array_code, check_fec, hamming_code,
                                       sc_array_code)
    assert list(fec._FEC_TABLE) == [LdpcCode, ScLdpcCode, StaircaseCode, ProductCode]
    ham = hamming_code(4)
    rows = {LdpcCode: (dict(code=array_code(4, 24, 31)), dict(window=5)),
            ScLdpcCode: (dict(code=sc_array_code(2, 4, 31, 12), window=5), dict(max_iter=8)),
            StaircaseCode: (dict(code=StaircaseCode(BchCode(5, 2, n=30), 4), window=3), dict(max_iter=8)),
            ProductCode: (dict(code=ProductCode(ham, ham)), dict(window=2))}
    for cls, (keys, required, check, decoder) in fec._FEC_TABLE.items():
        good, foreign = rows[cls]
        assert isinstance(good["code"], cls) and {"code", *required} == set(good) <= set(keys)         # code itself is what the row is found by
        assert callable(check) and callable(getattr(fec, decoder))
        (key, value), = foreign.items()
        assert key not in keys and any(key in row[0] for row in fec._FEC_TABLE.values())
        check_fec(good)
        with pytest.raises(ValueError):
            check_fec(dict(good, **foreign))
        for k in good:
            with pytest.raises(ValueError):
                check_fec({j: v for j, v in good.items() if j != k})
    check_fec(None)


def test_share_is_one_true_division_in_float64():
    from vae_equalizer_amd.fec import _share
    zero = _share(torch.zeros(2, 3, dtype=torch.int64), 0)
    assert zero.dtype == torch.float32 and zero.shape == (2,) and np.array_equal(zero.numpy(), np.zeros(2, np.float32))   # max(total, 1): no NaN
    got = _share(torch.tensor([[1, 2], [0, 0]]), 3).numpy()
    assert got.dtype == np.float32 and got[0] == np.float32(np.float64(3) / np.float64(3)) and got[1] == 0.0
    assert np.array_equal(got.view(np.uint32), np.array([1.0, 0.0], np.float32).view(np.uint32))
    third = _share(torch.tensor([[1]]), 3).numpy()
    assert np.array_equal(third.view(np.uint32), np.array([np.float32(1 / 3)]).view(np.uint32))           # the correctly rounded quotient
    assert _share(torch.tensor([[True, False, True, True]]), 4).item() == 0.75                            # a mask counts its set entries
