"""Drop-in for AWGN_channel/Eval_run_shaping_vaele.py: same constants, sweep order, result tensor and ``.mat`` schema
(:40, :60-69); sweep points are sharded over ranks (r mod world) and gathered once at the end."""
from datetime import datetime
from itertools import product

import scipy.io as io

mod = '64-QAM'          # Modulation Format: {4,16,64}-QAM
sps = 2                 # samples per symbol
channel = 'h1'          # 'h2'
M_vec = [25]            # taps of the estimated channel impulse response
N_train_vec = [350]     # length of training/updating batch in symbols
lr_optim_vec = [5e-3]
SNR_vec = [24]
nu_vec = [0]            # [0] [0.0270955] [0.0872449] [0.1222578]
iter = 20               # independent runs per setting
N_valid = 15000         # symbols per evaluation step
train_len = 1200        # training symbols per epoch
num_epochs = 500
epe = 2                 # epochs per evaluation

savePATH = ""
base_seed = None        # int -> reproducible runs; None = like the reference
info_metrics = False    # True: the .mat gains GMI, NGMI, AIR (bit per 2-D symbol) and BER (pre-FEC), each shaped like SER
generator = None        # None: "hip" (on-device generator vaeq_gen_awgn) for unseeded sweeps, "numpy" (reference-faithful host simulator) when base_seed is set
fec_metrics = None      # dict(code=fec.LdpcCode, t0=0, max_iter=20, alpha=0.75, depth=None, quant=None, outer=None; quant=dict(bits=5) decodes in fixed point and takes no alpha; outer=dict(code=fec.BchCode, ...) puts fec.bch_outer behind it, and the .mat also gains BER_outer and FER_outer): the .mat gains BER_post, FER, BER_pre_fec and fec_iters (mean over codewords; with code=fec.ScLdpcCode, which takes window, iters and test in place of max_iter, depth and quant: mean over the chains of a chain's total iteration count, and FER is the share of chains with errors) of the last validation's LLRs, each shaped like SER without its last axis
INFO_KEYS = ("GMI", "NGMI", "AIR", "BER")


def sweep_points():
    """The reference's loop nest (:43-58); note its SER has no nu axis, so later nu values overwrite earlier ones."""
    for (n, N_train), (l, lr), (m, M), (s, SNR), nu, i in product(enumerate(N_train_vec), enumerate(lr_optim_vec), enumerate(M_vec),
                                                                 enumerate(SNR_vec), nu_vec, range(iter)):
        yield (s, 0, 0, m, l, n, i), dict(N_train=N_train, lr=lr, M=M, SNR=SNR, nu=nu)


def main():
    from . import sweep
    from .func_VAELE_MQAM_shaping import run_awgn_batch

    keys, n_fec = INFO_KEYS if info_metrics else (), len(sweep.fec_keys(fec_metrics))

    def run_batch(shape, pts, seeds, device, seed):
        M, N_train = shape
        runs = [dict(SNR=p["SNR"], nu=p["nu"], lr_optim=p["lr"], seed=s) for p, s in zip(pts, seeds)]
        r = run_awgn_batch(runs, mod, sps, M, N_train, N_valid, train_len, num_epochs, epe, channel, device=device, generator=generator, seed=seed,
                           want_info=info_metrics, fec=fec_metrics)
        if fec_metrics is not None:
            return sweep.fec_rows(r, keys)                                        # per run: SER | keys | BER_post | FER | BER_pre_fec | fec_iters (| BER_outer | FER_outer)
        return sweep.info_rows(r, INFO_KEYS) if info_metrics else r               # per run: SER | GMI | NGMI | AIR | BER

    n_eval = num_epochs // epe
    out = sweep.run_sharded(list(sweep_points()), lambda p: (p["M"], p["N_train"]), run_batch, base_seed,
                            (len(SNR_vec), 1, 1, len(M_vec), len(lr_optim_vec), len(N_train_vec), iter),
                            (1 + len(keys) + n_fec, n_eval) if keys or n_fec else (n_eval,))
    if out is None:
        return None
    nu = nu_vec[-1]
    name = f"{savePATH}SERvsSNR_VAELE_shaping_{nu}_{channel}_{mod}_{sps}_{N_valid}_{epe}_{train_len}_{datetime.today().strftime('%y%m%d%H%M%S')}.mat"
    save_dict = {'SER': out[0].numpy(), 'SNR': SNR_vec, 'M': M_vec, 'lr': lr_optim_vec, 'N_train': N_train_vec, 'nu': nu_vec}
    save_dict.update({k: arr.numpy() for k, arr in zip(keys, out[1:])})
    save_dict.update({k: arr[..., -1].numpy() for k, arr in zip(sweep.fec_keys(fec_metrics), out[1 + len(keys):])})
    io.savemat(name, {'dict': save_dict})
    return name, save_dict

if __name__ == "__main__":
    main()
