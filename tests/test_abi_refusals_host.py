"""Which error code every size-taking entry point of include/vaeq.h returns for which refused arguments.

Every argument set below is refused on the host before any HIP call, so no device is needed (the library loads on a CPU-only host).  The
expected codes are literals recorded from the library before the C ABI's checks and launches were consolidated (csrc/vaeq_launch.h): they
pin the order of the checks (NULL before SHAPE before LDS where an entry point has that order, SHAPE first in the constant-modulus family),
the 160 KiB / 150 KiB ceiling each entry point has, and the exact size at which it trips (the VAE-NN ceilings sit behind the n_lev dispatch: only
their refused side is reachable without a launch).  A new baseline adds its rows here.
"""
import ctypes as C

import pytest

OK, NULL, SHAPE, LDS = 0, -1, -2, -3
P = 0xD0000                                                # a non-NULL "device pointer": never dereferenced by a refused call

# name -> (parameter names, argument set that would be accepted); pointers are P
SIG = {
    "vaeq_soft_demap": ("R N n_lev y amp var nu_sc q stream", (1, 64, 4, P, P, P, P, P, None)),
    "vaeq_dp_forward": ("R N sps M n_lev x W amp var nu_sc q y stream", (1, 64, 2, 25, 4, P, P, P, P, P, P, P, None)),
    "vaeq_dp_loss": ("R B sps M n_lev q x h amp P loss var_est stream", (1, 64, 2, 25, 4, P, P, P, P, P, P, P, None)),
    "vaeq_dp_loss_bwd": ("R B sps M n_lev q x h amp P g_up gq gh stream", (1, 64, 2, 25, 4, P, P, P, P, P, P, P, P, None)),
    "vaeq_dp_forward_bwd": ("R N sps M n_lev x q y gq gy amp var gW stream", (1, 64, 2, 25, 4, P, P, P, P, P, P, P, P, None)),
    "vaeq_awgn_forward": ("R N sps M n_lev x W amp amp_mean var q y stream", (1, 64, 2, 25, 4, P, P, P, P, P, P, P, None)),
    "vaeq_awgn_loss": ("R B sps M n_lev q x h amp P loss stream", (1, 64, 2, 25, 4, P, P, P, P, P, P, None)),
    "vaeq_awgn_loss_bwd": ("R B sps M n_lev q x h amp P g_up gq gh stream", (1, 64, 2, 25, 4, P, P, P, P, P, P, P, P, None)),
    "vaeq_awgn_forward_bwd": ("R N sps M n_lev x W amp amp_mean var gq gy gW stream", (1, 64, 2, 25, 4, P, P, P, P, P, P, P, P, None)),
    "vaeq_awgn_validate": ("R N sps M n_lev n_shift x W amp amp_mean var data y_ws ser shift stream",
                           (1, 2000, 2, 25, 4, 11, P, P, P, P, P, P, P, P, P, None)),
    "vaeq_awgn_validate_gen": ("R N sps M n_lev n_shift sig Ls power_ws snr_db sigma_fixed seed frame W amp amp_mean var data y_ws ser shift sigma_out stream",
                               (1, 2000, 2, 25, 4, 11, P, 4000, P, P, P, 1, 0, P, P, P, P, P, P, P, P, P, None)),
    "vaeq_dp_epilogue": ("R N n_lev batch_len q y tx amp var nu_sc ser shift rflag workspace stream", (1, 4000, 4, 0, P, P, P, P, P, P, P, P, P, P, None)),
    "vaeq_dp_epilogue_compact": ("R N n_lev batch_len eq dec y tx amp var nu_sc ser shift rflag stream",
                                 (1, 4000, 4, 0, P, P, P, P, P, P, P, P, P, P, None)),
    "vaeq_cma_epilogue": ("R N n_lev y tx amp var nu_sc ser shift rflag workspace stream", (1, 4000, 4, P, P, P, P, P, P, P, P, P, None)),
    "vaeq_nn_forward": ("R N sps M n_lev k1 k2 x theta bn_running q stream", (1, 64, 2, 25, 4, 25, 3, P, P, P, P, None)),
    "vaeq_nn_validate": ("R N sps M n_lev k1 k2 n_shift x theta bn_running amp data ser shift stream",
                         (1, 2000, 2, 25, 4, 25, 3, 11, P, P, P, P, P, P, P, None)),
    "vaeq_nn_enc_forward": ("R L sps n_lev k1 k2 batch_norm training x theta bn_running bn_saved q stream",
                            (1, 128, 2, 4, 25, 3, 1, 1, P, P, P, P, P, None)),
    "vaeq_nn_enc_backward": ("R L sps n_lev k1 k2 batch_norm training x theta q gq bn_stats g stream",
                             (1, 128, 2, 4, 25, 3, 1, 1, P, P, P, P, P, P, None)),
    "vaeq_cma": ("R N sps M mode batchlen symb_step rx R_mod h lr out e stream", (1, 4096, 2, 25, 1, 100, 10, P, 1.0, P, P, P, P, None)),
    "vaeq_cpe": ("R N M_ma y y_out stream", (1, 4096, 501, P, P, None)),
    "vaeq_awgn_cma": ("R N sps M update rx R_mod h lr loss out e stream", (1, 4096, 2, 25, 1, P, 1.0, P, P, P, P, P, None)),
    "vaeq_awgn_cma_validate": ("R N sps M n_lev n_shift rx h amp data ws ser shift cpe_out stream",
                               (1, 4096, 2, 25, 4, 11, P, P, P, P, P, P, P, P, None)),
    "vaeq_gen_dp_tx": ("R N N_conv sps n_lev Lg Ls Lrow ref_offset amp cdf g seed frame sig data stream",
                       (1, 100, 120, 2, 4, 21, 219, 256, 10, P, P, P, 1, 0, P, P, None)),
    "vaeq_gen_dp_disperse": ("R Ls fs tau_cd tau_pmd e0_re e0_im e1_re e1_im scale theta spec stream",
                             (1, 219, 1e9, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, P, P, None)),
    "vaeq_gen_dp_finish": ("R N sps Ls Lrow snr_db seed frame sig power_ws rx sigma_out stream", (1, 100, 2, 219, 256, P, 1, 0, P, P, P, P, None)),
    "vaeq_gen_dp_frame": ("R N N_conv sps n_lev Lg Ls Lrow ref_offset amp cdf g snr_db theta fs tau_cd tau_pmd e0_re e0_im e1_re e1_im seed frame "
                          "sig_ws power_ws rx data sigma_out stream",
                          (1, 100, 120, 2, 4, 21, 219, 256, 10, P, P, P, P, P, 1e9, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1, 0, P, P, P, P, P, None)),
    "vaeq_gen_awgn": ("R N N_conv sps n_lev Lg Ls ref_offset amp cdf g snr_db seed frame sig_ws power_ws rx data sigma_out sigma_fixed stream",
                      (1, 100, 120, 2, 4, 21, 219, 10, P, P, P, P, 1, 0, P, P, P, P, P, P, None)),
    "vaeq_gen_awgn_clean": ("R N N_conv sps n_lev Lg Ls ref_offset amp cdf g seed frame sig power_ws data stream",
                            (1, 100, 120, 2, 4, 21, 219, 10, P, P, P, 1, 0, P, P, P, None)),
    "vaeq_awgn_lmmse_eval": ("R N sps n_lev K n_shift n_cut rx taps amp data ws ser shift dec out stream",
                             (1, 4096, 1, 4, 32, 11, 0, P, P, P, P, P, P, P, P, P, None)),
    "vaeq_awgn_dfe": ("R N sps n_lev K1 K2 C W n_shift n_cut rx ff_taps fb_taps amp init_dec data ws dec ser shift repairs ff_out stream",
                      (1, 4096, 1, 4, 32, 3, 8, 16, 11, 0, P, P, P, P, P, P, P, P, P, P, P, P, None)),
    "vaeq_stream_copy": ("dst src bytes stream", (P, P, 1024, None)),
    # size queries: the "code" is the (negative) return value
    "vaeq_gen_dp_power_parts": ("Lrow", (20480,)),
    "vaeq_dp_epilogue_ws_bytes": ("R N", (1, 4000)),
    "vaeq_awgn_lmmse_eval_ws_bytes": ("R N K", (1, 4096, 32)),
    "vaeq_awgn_dfe_ws_bytes": ("R N C", (1, 4096, 8)),
    "vaeq_dp_lds_bytes": ("B sps M n_lev", (64, 2, 25, 4)),
    "vaeq_dp_resident_runs": ("B sps M n_lev threads", (64, 2, 25, 4, 0)),
    "vaeq_awgn_lds_bytes": ("B sps M n_lev", (64, 2, 25, 4)),
    "vaeq_nn_param_count": ("M n_lev k1 k2 batch_norm", (25, 4, 25, 3, 0)),
    "vaeq_nn_lds_bytes": ("B sps M n_lev k1 k2 batch_norm", (64, 2, 25, 4, 25, 3, 0)),
    "vaeq_nn_enc_param_count": ("n_lev k1 k2 batch_norm", (4, 25, 3, 0)),
    "vaeq_nn_enc_lds_bytes": ("L sps n_lev k1 k2 batch_norm", (128, 2, 4, 25, 3, 0)),
    "vaeq_awgn_cma_validate_ws_bytes": ("R N sps", (1, 4096, 2)),
}

# the three training loops take a struct: field overrides on an argument set that would be accepted (every pointer P)
STRUCT = {
    "vaeq_dp_train": ("DPArgs", dict(R=1, n_frames=1, steps=1, B=64, sps=2, M=25, n_lev=4, stride_sym=64, keep_off=0, keep_len=64, S=128)),
    "vaeq_dp_step_debug": ("DPArgs", dict(R=1, n_frames=1, steps=1, B=64, sps=2, M=25, n_lev=4, stride_sym=64, keep_off=0, keep_len=64, S=128)),
    "vaeq_awgn_train": ("AWGNArgs", dict(R=1, steps=1, B=64, sps=2, M=25, n_lev=4, S=128)),
    "vaeq_nn_train": ("NNArgs", dict(R=1, steps=1, B=64, sps=2, M=25, n_lev=4, k1=25, k2=3, S=128)),
}

# (entry point, {argument: value, ...} or "empty" = R 0 with every pointer NULL, expected code)
CASES = [
    # ---- an empty batch owns no memory
    *[(f, "empty", OK) for f in SIG if SIG[f][0].startswith("R ") and not f.endswith("_ws_bytes")],
    ("vaeq_dp_train", "empty", OK), ("vaeq_awgn_train", "empty", OK), ("vaeq_nn_train", "empty", OK),
    # ---- one required pointer NULL
    ("vaeq_soft_demap", dict(y=None), NULL), ("vaeq_soft_demap", dict(q=None), NULL),
    ("vaeq_dp_forward", dict(x=None), NULL), ("vaeq_dp_forward", dict(y=None), NULL),
    ("vaeq_dp_loss", dict(q=None), NULL), ("vaeq_dp_loss", dict(P=None), NULL), ("vaeq_dp_loss", dict(var_est=None), NULL),
    ("vaeq_dp_loss_bwd", dict(g_up=None), NULL), ("vaeq_dp_loss_bwd", dict(P=None), NULL),
    ("vaeq_dp_forward_bwd", dict(gW=None), NULL), ("vaeq_dp_forward_bwd", dict(y=None), NULL),
    ("vaeq_awgn_forward", dict(W=None), NULL), ("vaeq_awgn_forward", dict(y=None), NULL),
    ("vaeq_awgn_loss", dict(loss=None), NULL), ("vaeq_awgn_loss_bwd", dict(gh=None), NULL), ("vaeq_awgn_forward_bwd", dict(gq=None), NULL),
    ("vaeq_awgn_validate", dict(data=None), NULL), ("vaeq_awgn_validate_gen", dict(sig=None), NULL),
    ("vaeq_awgn_validate_gen", dict(snr_db=None, sigma_fixed=None), NULL),
    ("vaeq_dp_epilogue", dict(workspace=None), NULL), ("vaeq_dp_epilogue_compact", dict(dec=None), NULL), ("vaeq_cma_epilogue", dict(tx=None), NULL),
    ("vaeq_nn_forward", dict(theta=None), NULL), ("vaeq_nn_validate", dict(amp=None), NULL),
    ("vaeq_nn_enc_forward", dict(q=None), NULL), ("vaeq_nn_enc_forward", dict(training=0, bn_running=None), NULL),
    ("vaeq_nn_enc_backward", dict(bn_stats=None), NULL),
    ("vaeq_cma", dict(rx=None), NULL), ("vaeq_cpe", dict(y_out=None), NULL), ("vaeq_awgn_cma", dict(loss=None), NULL),
    ("vaeq_awgn_cma_validate", dict(ser=None), NULL),
    ("vaeq_dp_train", dict(rx=None), NULL), ("vaeq_dp_train", dict(lr_h=None), NULL), ("vaeq_dp_step_debug", dict(gW=None), NULL),
    ("vaeq_awgn_train", dict(adam_xh=None), NULL), ("vaeq_nn_train", dict(theta=None), NULL), ("vaeq_nn_train", dict(batch_norm=1, bn_running=None), NULL),
    # ---- NULL is reported before SHAPE (and SHAPE before NULL in the constant-modulus family)
    ("vaeq_dp_loss", dict(q=None, M=24), NULL), ("vaeq_awgn_loss_bwd", dict(gh=None, sps=0), NULL), ("vaeq_dp_forward", dict(x=None, M=65), NULL),
    ("vaeq_awgn_train", dict(rx=None, M=24), NULL), ("vaeq_nn_forward", dict(q=None, k1=24), NULL),
    ("vaeq_cma", dict(rx=None, M=24), SHAPE), ("vaeq_cpe", dict(y=None, M_ma=500), SHAPE), ("vaeq_awgn_cma", dict(rx=None, M=24), SHAPE),
    ("vaeq_awgn_cma_validate", dict(rx=None, n_shift=10), SHAPE), ("vaeq_awgn_cma", dict(R=0, M=24), SHAPE),
    # ---- even M, M = 65, sps = 0
    *[(f, dict(M=m), SHAPE) for m in (24, 65, 0) for f in (
        "vaeq_dp_forward", "vaeq_dp_loss", "vaeq_dp_loss_bwd", "vaeq_dp_forward_bwd", "vaeq_awgn_forward", "vaeq_awgn_loss", "vaeq_awgn_loss_bwd",
        "vaeq_awgn_forward_bwd", "vaeq_awgn_validate", "vaeq_awgn_validate_gen", "vaeq_nn_forward", "vaeq_nn_validate", "vaeq_cma", "vaeq_awgn_cma",
        "vaeq_awgn_cma_validate", "vaeq_dp_train", "vaeq_awgn_train", "vaeq_nn_train", "vaeq_dp_lds_bytes", "vaeq_dp_resident_runs",
        "vaeq_awgn_lds_bytes", "vaeq_nn_param_count", "vaeq_nn_lds_bytes")],
    *[(f, dict(sps=0), SHAPE) for f in (
        "vaeq_dp_forward", "vaeq_dp_loss", "vaeq_dp_loss_bwd", "vaeq_dp_forward_bwd", "vaeq_awgn_forward", "vaeq_awgn_loss", "vaeq_awgn_loss_bwd",
        "vaeq_awgn_forward_bwd", "vaeq_awgn_validate", "vaeq_awgn_validate_gen", "vaeq_nn_forward", "vaeq_nn_validate", "vaeq_nn_enc_forward",
        "vaeq_nn_enc_backward", "vaeq_cma", "vaeq_awgn_cma", "vaeq_awgn_cma_validate", "vaeq_dp_train", "vaeq_awgn_train", "vaeq_nn_train",
        "vaeq_dp_lds_bytes", "vaeq_dp_resident_runs", "vaeq_awgn_lds_bytes", "vaeq_nn_lds_bytes", "vaeq_nn_enc_lds_bytes",
        "vaeq_awgn_cma_validate_ws_bytes")],
    # ---- n_lev = 3
    *[(f, dict(n_lev=3), SHAPE) for f in (
        "vaeq_soft_demap", "vaeq_dp_forward", "vaeq_dp_loss", "vaeq_dp_loss_bwd", "vaeq_dp_forward_bwd", "vaeq_awgn_forward", "vaeq_awgn_loss",
        "vaeq_awgn_loss_bwd", "vaeq_awgn_forward_bwd", "vaeq_awgn_validate", "vaeq_awgn_validate_gen", "vaeq_dp_epilogue", "vaeq_dp_epilogue_compact",
        "vaeq_cma_epilogue", "vaeq_nn_forward", "vaeq_nn_validate", "vaeq_nn_enc_forward", "vaeq_nn_enc_backward", "vaeq_awgn_cma_validate",
        "vaeq_dp_train", "vaeq_awgn_train", "vaeq_nn_train", "vaeq_dp_lds_bytes", "vaeq_dp_resident_runs", "vaeq_awgn_lds_bytes",
        "vaeq_nn_param_count", "vaeq_nn_lds_bytes", "vaeq_nn_enc_param_count", "vaeq_nn_enc_lds_bytes")],
    # ---- negative R; other sizes out of range
    *[(f, dict(R=-1), SHAPE) for f in ("vaeq_soft_demap", "vaeq_dp_forward", "vaeq_dp_loss", "vaeq_dp_loss_bwd", "vaeq_dp_forward_bwd", "vaeq_awgn_forward",
                                       "vaeq_awgn_loss", "vaeq_awgn_loss_bwd", "vaeq_awgn_forward_bwd", "vaeq_awgn_validate", "vaeq_nn_forward", "vaeq_cma",
                                       "vaeq_cpe", "vaeq_awgn_cma", "vaeq_dp_train", "vaeq_awgn_train", "vaeq_nn_train")],
    ("vaeq_awgn_validate", dict(N=63), SHAPE), ("vaeq_awgn_validate", dict(N=65537), SHAPE), ("vaeq_awgn_validate", dict(n_shift=0), SHAPE),
    ("vaeq_awgn_validate_gen", dict(sps=1), SHAPE), ("vaeq_awgn_validate_gen", dict(M=11), SHAPE), ("vaeq_awgn_validate_gen", dict(Ls=3999), SHAPE),
    ("vaeq_dp_epilogue", dict(N=10), SHAPE), ("vaeq_dp_epilogue", dict(batch_len=7), SHAPE), ("vaeq_dp_epilogue_compact", dict(batch_len=-1), SHAPE),
    ("vaeq_cma_epilogue", dict(N=10), SHAPE), ("vaeq_cpe", dict(N=12801), SHAPE), ("vaeq_cpe", dict(M_ma=500), SHAPE),
    ("vaeq_cma", dict(mode=2), SHAPE), ("vaeq_cma", dict(batchlen=4097), SHAPE), ("vaeq_cma", dict(N=99), SHAPE),
    ("vaeq_awgn_cma", dict(sps=9), SHAPE), ("vaeq_awgn_cma", dict(N=4095), SHAPE), ("vaeq_awgn_cma_validate", dict(N=2000), SHAPE),
    ("vaeq_nn_forward", dict(k2=11), SHAPE), ("vaeq_nn_validate", dict(N=63), SHAPE), ("vaeq_nn_enc_forward", dict(L=1), SHAPE),
    ("vaeq_nn_enc_backward", dict(L=0), SHAPE), ("vaeq_nn_train", dict(S=127), SHAPE), ("vaeq_awgn_train", dict(S=127), SHAPE),
    ("vaeq_dp_train", dict(S=127), SHAPE), ("vaeq_dp_train", dict(keep_len=65), SHAPE), ("vaeq_dp_train", dict(threads=1, sps=3, S=192), SHAPE),
    ("vaeq_dp_step_debug", dict(steps=2), SHAPE), ("vaeq_dp_resident_runs", dict(threads=1, sps=3), SHAPE), ("vaeq_dp_resident_runs", dict(threads=7, sps=3), SHAPE),
    # ---- the loss family wants a minibatch longer than the FIR: B <= 2 (M / 2)
    *[(f, dict(B=24), SHAPE) for f in ("vaeq_dp_loss", "vaeq_dp_loss_bwd", "vaeq_awgn_loss", "vaeq_awgn_loss_bwd", "vaeq_awgn_train", "vaeq_nn_train",
                                       "vaeq_awgn_lds_bytes", "vaeq_nn_lds_bytes")],
    ("vaeq_dp_lds_bytes", dict(B=12), SHAPE),                  # (the DP training loop takes the reference's short minibatches: only nm > 0)
    ("vaeq_dp_train", dict(B=12, keep_len=12, stride_sym=12), SHAPE),
    # ---- LDS ceilings: the first refused size (LDS), and the last one not refused for its size (n_lev = 3: SHAPE from the dispatch behind the LDS check)
    ("vaeq_dp_loss", dict(B=5081), LDS), ("vaeq_dp_loss", dict(B=5080, n_lev=3), SHAPE),                                   # 160 KiB
    ("vaeq_dp_loss_bwd", dict(B=2547), LDS), ("vaeq_dp_loss_bwd", dict(B=2546, n_lev=3), SHAPE),                           # 160 KiB
    ("vaeq_dp_forward_bwd", dict(N=10241), LDS), ("vaeq_dp_forward_bwd", dict(N=10240, n_lev=3), SHAPE),                   # 160 KiB
    ("vaeq_awgn_loss", dict(B=9601), LDS), ("vaeq_awgn_loss", dict(B=9600, n_lev=3), SHAPE),                               # 150 KiB
    ("vaeq_awgn_loss_bwd", dict(B=4807), LDS), ("vaeq_awgn_loss_bwd", dict(B=4806, n_lev=3), SHAPE),                       # 150 KiB
    ("vaeq_awgn_forward_bwd", dict(N=9601), LDS), ("vaeq_awgn_forward_bwd", dict(N=9600, n_lev=3), SHAPE),                 # 150 KiB
    ("vaeq_dp_train", dict(B=8192, keep_len=8192, stride_sym=8192, S=16384), LDS),
    ("vaeq_awgn_train", dict(B=8192, S=16384), LDS),
    ("vaeq_nn_train", dict(B=8192, S=16384), LDS),
    ("vaeq_nn_enc_backward", dict(L=(1 << 20) + 1), LDS), ("vaeq_nn_enc_forward", dict(L=(1 << 20) + 1), LDS),
    # The VAE-NN ceilings sit behind the n_lev dispatch, so only their refused side can be reached without a launch.  The eval layout of a
    # 255-symbol tile at n_lev 8, sps 6, k2 3 takes 153 488 B (k1 9), 157 712 B (k1 25), 163 248 B (k1 47), 164 048 B (k1 49).
    ("vaeq_nn_forward", dict(n_lev=8, sps=6, k1=49), LDS),                                                                  # 160 KiB
    ("vaeq_nn_validate", dict(n_lev=8, sps=6, k1=9, N=113), LDS),          # 150 KiB: layout + the decisions, N rounded up to 16 (N = 112 fits)
    ("vaeq_nn_validate", dict(n_lev=8, sps=6, k1=25, N=64), LDS),          # between 150 and 160 KiB
    # the encoder operators keep a run's whole input in LDS: vaeq_nn_enc_lds_bytes is their formula (160 KiB = 163 840 B)
    ("vaeq_nn_enc_lds_bytes", dict(L=792, batch_norm=1), 163792), ("vaeq_nn_enc_lds_bytes", dict(L=793, batch_norm=1), 163856),
    ("vaeq_nn_enc_lds_bytes", dict(L=1216), 162768), ("vaeq_nn_enc_lds_bytes", dict(L=1217), 163856),
    ("vaeq_nn_enc_backward", dict(L=793), LDS), ("vaeq_nn_enc_backward", dict(L=1217, batch_norm=0), LDS), ("vaeq_nn_enc_forward", dict(L=793), LDS),
    # ---- the channel simulators: NULL before SHAPE; the 'valid' convolution length Ls = sps (N_conv - 1) + 1 - Lg + 1, rows of Lrow >= Ls
    ("vaeq_gen_dp_tx", dict(amp=None), NULL), ("vaeq_gen_dp_tx", dict(sig=None), NULL), ("vaeq_gen_dp_tx", dict(amp=None, sps=0), NULL),
    *[("vaeq_gen_dp_tx", c, SHAPE) for c in (dict(R=-1), dict(N=0), dict(sps=0), dict(n_lev=3), dict(Lg=0), dict(Lg=97), dict(ref_offset=-1),
                                             dict(ref_offset=21), dict(Ls=218), dict(Lrow=218), dict(N=110, ref_offset=0))],
    ("vaeq_gen_dp_disperse", dict(theta=None), NULL), ("vaeq_gen_dp_disperse", dict(theta=None, Ls=0), NULL),
    ("vaeq_gen_dp_disperse", dict(Ls=0), SHAPE), ("vaeq_gen_dp_disperse", dict(R=-1), SHAPE),
    ("vaeq_gen_dp_finish", dict(rx=None), NULL), ("vaeq_gen_dp_finish", dict(snr_db=None, sps=0), NULL),
    *[("vaeq_gen_dp_finish", c, SHAPE) for c in (dict(R=-1), dict(N=0), dict(sps=0), dict(Ls=199), dict(Lrow=218))],
    ("vaeq_gen_dp_frame", dict(theta=None), NULL), ("vaeq_gen_dp_frame", dict(snr_db=None), NULL), ("vaeq_gen_dp_frame", dict(amp=None, n_lev=3), NULL),
    *[("vaeq_gen_dp_frame", c, SHAPE) for c in (dict(R=-1), dict(sps=0), dict(n_lev=3), dict(Lg=97), dict(Ls=218), dict(Lrow=218))],
    ("vaeq_gen_dp_power_parts", dict(Lrow=0), SHAPE), ("vaeq_gen_dp_power_parts", dict(Lrow=-5), SHAPE),
    ("vaeq_gen_awgn", dict(amp=None), NULL), ("vaeq_gen_awgn", dict(snr_db=None, sigma_fixed=None), NULL), ("vaeq_gen_awgn", dict(rx=None, n_lev=3), NULL),
    ("vaeq_gen_awgn", dict(sps=3, sig_ws=None), NULL),         # the clean signal goes through sig_ws unless sps == 2
    *[("vaeq_gen_awgn", c, SHAPE) for c in (dict(R=-1), dict(sps=0), dict(n_lev=3), dict(Lg=97), dict(Ls=218), dict(ref_offset=21))],
    ("vaeq_gen_awgn_clean", dict(power_ws=None), NULL), ("vaeq_gen_awgn_clean", dict(sig=None, sps=1), NULL),
    *[("vaeq_gen_awgn_clean", c, SHAPE) for c in (dict(R=-1), dict(sps=1), dict(sps=0), dict(n_lev=3), dict(Ls=218))],
    ("vaeq_dp_epilogue_ws_bytes", dict(R=-1), SHAPE), ("vaeq_dp_epilogue_ws_bytes", dict(N=-1), SHAPE),
    # ---- the known-channel baselines: SHAPE before the empty batch and before NULL, like the constant-modulus family
    ("vaeq_awgn_lmmse_eval", dict(rx=None), NULL), ("vaeq_awgn_lmmse_eval", dict(out=None, ws=None), NULL),
    ("vaeq_awgn_lmmse_eval", dict(rx=None, K=31), SHAPE), ("vaeq_awgn_lmmse_eval", dict(R=0, sps=2), SHAPE),
    *[("vaeq_awgn_lmmse_eval", c, SHAPE) for c in (dict(R=-1), dict(sps=2), dict(n_lev=3), dict(K=0), dict(K=66), dict(K=31), dict(n_shift=0),
                                                   dict(n_shift=65), dict(n_cut=-1), dict(n_shift=25), dict(N=1032))],
    *[("vaeq_awgn_lmmse_eval_ws_bytes", c, SHAPE) for c in (dict(R=-1), dict(N=0), dict(K=0), dict(K=65))],
    ("vaeq_awgn_dfe", dict(rx=None), NULL), ("vaeq_awgn_dfe", dict(data=None), NULL), ("vaeq_awgn_dfe", dict(ser=None, n_shift=0, rx=None), NULL),
    ("vaeq_awgn_dfe", dict(rx=None, K2=0), SHAPE), ("vaeq_awgn_dfe", dict(R=0, C=0), SHAPE),
    *[("vaeq_awgn_dfe", c, SHAPE) for c in (dict(R=-1), dict(sps=2), dict(n_lev=3), dict(K1=65), dict(K2=0), dict(K2=11), dict(C=0), dict(C=8193),
                                            dict(W=-1), dict(n_shift=0), dict(N=1032), dict(K2=10, C=1000))],         # (the last: chunks of 5 symbols < K2),
    *[("vaeq_awgn_dfe_ws_bytes", c, SHAPE) for c in (dict(R=-1), dict(N=0), dict(C=0), dict(C=8193))],
    # ---- the copy probe: 16-byte granules at 16-byte addresses
    ("vaeq_stream_copy", dict(dst=None), NULL), ("vaeq_stream_copy", dict(src=None, bytes=8), NULL), ("vaeq_stream_copy", dict(bytes=0), OK),
    ("vaeq_stream_copy", dict(bytes=8), SHAPE), ("vaeq_stream_copy", dict(bytes=-16), SHAPE), ("vaeq_stream_copy", dict(src=P + 4), SHAPE),
]


def _call(nat, fn, change):
    L = nat.lib()
    f = getattr(L, fn)
    if fn in STRUCT:
        cls, fields = STRUCT[fn]
        cls = getattr(nat, cls)
        a = cls()
        for name, ctype in cls._fields_:
            if ctype is C.c_void_p:
                setattr(a, name, P)
        for k, v in fields.items():
            setattr(a, k, v)
        extra = dict(gW=P, gh=P)
        if change == "empty":
            a = cls()
        else:
            for k, v in change.items():
                if k in extra:
                    extra[k] = v
                else:
                    setattr(a, k, v)
        if fn == "vaeq_dp_step_debug":
            return f(C.byref(a), extra["gW"], extra["gh"], None)
        return f(C.byref(a), None)
    names, base = SIG[fn]
    names = names.split()
    assert len(names) == len(base) == len(f.argtypes), fn
    args = list(base)
    if change == "empty":
        args = [None if v == P else v for v in args]
        args[0] = 0
    else:
        for k, v in change.items():
            args[names.index(k)] = v
    return f(*args)


def _id(case):
    fn, change, _ = case
    return fn[5:] + "-" + (change if isinstance(change, str) else ",".join("%s=%s" % kv for kv in change.items()))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_refusal_code(case):
    from vae_equalizer_amd import _native as nat
    fn, change, expected = case
    assert _call(nat, fn, change) == expected
