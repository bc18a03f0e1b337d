"""Drop-in for AWGN_channel/Eval_run_vaenn.py: same constants, sweep order, result tensor and ``.mat`` schema (:36, :58-68); sweep
points are sharded over ranks (r mod world) and gathered once at the end."""
from datetime import datetime
from itertools import product

import scipy.io as io

mod = '64-QAM'          # Modulation Format: {4,16,64}-QAM
sps = 2                 # samples per symbol
net_type_vec = ['Net']  # ['Net_BN'] # topology
channel = 'h1'          # 'h2'
M_vec = [25]            # taps of the estimated channel impulse response
k1_vec, k2_vec = [25], [3]  # kernel size (of layer1, layer2)
batch_len_vec = [300]   # length of training/updating batch in symbols
lr_optim_vec = [4e-3]
SNR_vec = [24]
iter = 3                # independent runs per setting
N_valid = 15000         # symbols per evaluation step
train_len = 4000        # training symbols per epoch
num_epochs = 500
epe = 2                 # epochs per evaluation

savePATH = ""
base_seed = None        # int -> reproducible runs; None = like the reference
info_metrics = False    # True: the .mat gains GMI, NGMI, AIR (bit per 2-D symbol) and BER (pre-FEC), each shaped like SER
generator = "hip"       # "hip": on-device channel model; "numpy": host restatement per run
fec_metrics = None      # dict(code=fec.LdpcCode, t0=0, max_iter=20, alpha=0.75, depth=None, quant=None, outer=None; quant=dict(bits=5) decodes in fixed point and takes no alpha; outer=dict(code=fec.BchCode, ...) puts fec.bch_outer behind it, and the .mat also gains BER_outer and FER_outer): the .mat gains BER_post, FER, BER_pre_fec and fec_iters (mean over codewords; with code=fec.ScLdpcCode, which takes window, iters and test in place of max_iter, depth and quant: mean over the chains of a chain's total iteration count, and FER is the share of chains with errors) of the last validation's LLRs, each shaped like SER without its last axis
INFO_KEYS = ("GMI", "NGMI", "AIR", "BER")


def sweep_points():
    """The reference's loop nest (:38-56) for one net_type."""
    for (n, batch_len), (l, lr), (m, M), (a, k1), (b, k2), (s, SNR), i in product(enumerate(batch_len_vec), enumerate(lr_optim_vec),
                                                                                  enumerate(M_vec), enumerate(k1_vec), enumerate(k2_vec),
                                                                                  enumerate(SNR_vec), range(iter)):
        yield (s, b, a, m, l, n, i), dict(batch_len=batch_len, lr=lr, M=M, k1=k1, k2=k2, SNR=SNR)


def main():
    from . import sweep
    from .func_VAENN_MQAM import run_vaenn_batch

    keys, n_fec = INFO_KEYS if info_metrics else (), len(sweep.fec_keys(fec_metrics))
    name = save_dict = None
    for j, net_type in enumerate(net_type_vec):
        def run_batch(shape, pts, seeds, device, seed):
            M, k1, k2, batch_len = shape
            runs = [dict(SNR=p["SNR"], lr_optim=p["lr"], seed=s) for p, s in zip(pts, seeds)]
            r = run_vaenn_batch(runs, mod, sps, M, k1, k2, batch_len, N_valid, train_len, num_epochs, epe, channel, device=device,
                                generator=generator, seed=seed, net_type=net_type, want_info=info_metrics, fec=fec_metrics)
            if fec_metrics is not None:
                return sweep.fec_rows(r, keys)                                        # per run: SER | keys | BER_post | FER | BER_pre_fec | fec_iters (| BER_outer | FER_outer)
            return sweep.info_rows(r, INFO_KEYS) if info_metrics else r           # per run: SER | GMI | NGMI | AIR | BER

        n_eval = num_epochs // epe
        out = sweep.run_sharded(list(sweep_points()), lambda p: (p["M"], p["k1"], p["k2"], p["batch_len"]), run_batch, base_seed,
                                (len(SNR_vec), len(k2_vec), len(k1_vec), len(M_vec), len(lr_optim_vec), len(batch_len_vec), iter),
                                (1 + len(keys) + n_fec, n_eval) if keys or n_fec else (n_eval,),
                                batch_offset=1000 * net_type_vec.index(net_type), announce=j == 0)
        if out is None:
            continue
        name = f"{savePATH}SERvsSNR_{net_type}_{channel}_{mod}_{sps}_{N_valid}_{epe}_{train_len}_{datetime.today().strftime('%y%m%d%H%M%S')}.mat"
        save_dict = {'SER': out[0].numpy(), 'SNR': SNR_vec, 'k2': k2_vec, 'k1': k1_vec, 'M': M_vec, 'lr': lr_optim_vec, 'N_train': batch_len_vec}
        save_dict.update({k: arr.numpy() for k, arr in zip(keys, out[1:])})
        save_dict.update({k: arr[..., -1].numpy() for k, arr in zip(sweep.fec_keys(fec_metrics), out[1 + len(keys):])})
        io.savemat(name, {'dict': save_dict})
    return (name, save_dict) if sweep.dist_info()[0] == 0 else None

if __name__ == "__main__":
    main()
