"""The epoch loop of the AWGN scripts (AWGN_channel/func_VAELE_MQAM_shaping.py:291-322, func_CMA_MQAM_shaping.py:213-232,
func_VAENN_MQAM.py:266-301) for R runs at once: per epoch one training frame and one training call, on evaluated epochs one validation.  The three
batch runners differ in their tables, their engine and their host channel model; they hand those in as plain callables."""
import torch

from . import channel as ch
from .dp_runs import _host_pool, fresh_seed
from .engine import INFO_FLOAT, INFO_INT
from .fec import check_fec, fec_figures


def check_generator(generator):
    """-> generator, or ValueError: the runners ask before they allocate or launch anything."""
    if generator not in ("hip", "numpy"):
        raise ValueError(f"unknown generator {generator!r}")
    return generator


def run_awgn_epochs(R, device, num_epochs, epe, N_train, N_valid, train, validate, generator, seed, gen_args, host, seeded, verbose=False,
                    want_info=False, want_llr=False, fec=None, **gen_kw):
    """train(rx[R,2,N_train*sps]) -> loss[R] (device; only read when verbose); validate(draw, N_valid) -> (SER[R], shift[R], info dict or None);
    validate(draw, N_valid, True), asked for the last evaluated validation when want_llr or fec is on -> (SER, shift, info dict, llr dict): the
    info call runs for its hyp whether or not want_info is on, then the LLR call on the same output and shift; llr dict =
    dict(llr[R,2b,N_valid] f32, bits[R,2b,N_valid] int8 = label_bits of the validation's TX data, hyp[R]).

    draw(N, clean=False) -> (rx[R,2,N*sps] f32, data[R,2,N] f16) on ``device``, and counts the frames it has drawn:
      "hip"   frame k of the on-device generator, ch.generate_awgn_batch_hip(R, N, *gen_args, device, seed, k, **gen_kw) (seed None: fresh
              entropy); clean=True draws frame k with ch.generate_awgn_clean_batch_hip instead and returns its CleanAwgnFrame;
      "numpy" host(N, i) -> (rx, data) on the CPU for every run i, concurrently when R > 1 and ``seeded`` (every run owns its random streams;
              unseeded runs share numpy's global stream and stay sequential).
    Epoch e is evaluated when e % epe == 0 and e // epe < num_epochs // epe (:308-318).  Nothing is read back before the end unless verbose.
    Returns SER_valid[R, num_epochs // epe] (CPU float32); with want_info (SER_valid, info), info[k][R, num_epochs // epe] on the CPU.
    want_llr / fec (fec.fec_figures' dict): (SER_valid, info or None, extras) with extras["llr"] = the last evaluated validation's llr dict
    (only with want_llr) and extras["fec"] = fec.ldpc_decode's figures of it (only with fec), both on the device.  A quant dict in fec decodes in fixed point (vaeq_ldpc_decode_q).  A bad fec dict is a
    ValueError before anything is allocated or launched."""
    check_generator(generator)
    check_fec(fec)
    soft = want_llr or fec is not None
    seed = fresh_seed() if seed is None else seed                               # Philox key of the device generator
    drawn = [0]

    def draw(N, clean=False):
        if generator == "hip":
            drawn[0] += 1
            fn = ch.generate_awgn_clean_batch_hip if clean else ch.generate_awgn_batch_hip
            return fn(R, N, *gen_args, device, seed, drawn[0] - 1, **gen_kw)
        pairs = list(_host_pool().map(lambda i: host(N, i), range(R))) if R > 1 and seeded else [host(N, i) for i in range(R)]
        return torch.stack([p[0] for p in pairs]).to(device), torch.stack([p[1] for p in pairs]).to(device)

    n_eval = num_epochs // epe
    SER_dev = torch.empty(R, max(n_eval, 1), dtype=torch.float32, device=device)
    info_dev = {k: torch.empty(R, max(n_eval, 1), dtype=torch.float32 if k in INFO_FLOAT else torch.int64, device=device)
                for k in INFO_FLOAT + INFO_INT} if want_info else None
    extras = {}
    for epoch in range(num_epochs):
        rx, _ = draw(N_train)
        loss = train(rx)
        if epoch % epe == 0 and epoch // epe < n_eval:
            if soft and epoch // epe == n_eval - 1:
                ser, sh, info, llr = validate(draw, N_valid, True)
                if want_llr:
                    extras["llr"] = llr
                if fec is not None:
                    extras["fec"] = fec_figures(llr, fec)
            else:
                ser, sh, info = validate(draw, N_valid)
            SER_dev[:, epoch // epe] = ser
            if want_info:
                for k, v in info.items():
                    info_dev[k][:, epoch // epe] = v
            if verbose:
                loss_h, ser_h, sh_h = loss.cpu(), ser.cpu(), sh.cpu()
                for i in range(R):
                    tag = f"[run {i}] " if R > 1 else ""
                    print(f"{tag}{epoch}", loss_h[i].item(), int(sh_h[i]), '\t\t\t\t\t\tSER = ', ser_h[i].item())
    info_cpu = {k: v[:, :n_eval].cpu() for k, v in info_dev.items()} if want_info else None
    if soft:
        return SER_dev[:, :n_eval].cpu(), info_cpu, extras
    if want_info:
        return SER_dev[:, :n_eval].cpu(), info_cpu
    return SER_dev[:, :n_eval].cpu()


def first_run(out, want_info=False):
    """A one-run batch's result without its run axis: what the processing() wrappers return."""
    return (out[0][0], {k: v[0] for k, v in out[1].items()}) if want_info else out[0]
