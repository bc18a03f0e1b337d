"""Sharding of an embarrassingly parallel parameter sweep over the GPUs of one node.

Run index r goes to rank r % world_size; every rank trains its runs with no communication, then ONE all_gather of
the per-run result rows (RCCL over xGMI when the backend is ``nccl``; ``gloo`` in the CPU tests) reassembles the
full result tensors on every rank.
"""
import os

import torch
import torch.distributed as dist


def dist_info():
    """(rank, world_size, local_rank) from torch.distributed if initialised, else from the launcher's environment."""
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size(), int(os.environ.get("LOCAL_RANK", 0))
    return int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("LOCAL_RANK", 0))


def init_distributed(backend=None):
    """Initialise the process group when launched by torch.distributed.run with WORLD_SIZE > 1 (one process per GPU).
    VAEQ_FORCE_COLLECTIVE=1 initialises it at WORLD_SIZE = 1 as well (under torch.distributed.run --nproc-per-node 1), so that RCCL's
    initialisation and the gather's collective run on a one-GPU box exactly as they do on N GPUs (gather_rows)."""
    world = int(os.environ.get("WORLD_SIZE", 1))
    force = bool(os.environ.get("VAEQ_FORCE_COLLECTIVE")) and "RANK" in os.environ
    if (world > 1 or force) and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend is None:
            backend = os.environ.get("VAEQ_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        if backend == "nccl":
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
        dist.init_process_group(backend=backend)
    return dist_info()


def device_for_rank(local_rank, world):
    """cuda:LOCAL_RANK (one process per GPU); VAEQ_SINGLE_DEVICE=1 maps every rank to cuda:0 to rehearse N > 1 on a one-GPU box."""
    if os.environ.get("VAEQ_SINGLE_DEVICE") or os.environ.get("VAEQ_BENCH_SINGLE_DEVICE"):
        return torch.device("cuda", 0)
    return torch.device("cuda", local_rank if world > 1 else torch.cuda.current_device())


def stream_seed(base_seed, rank, batch_index=0):
    """Key of a rank's device-generator streams for one batch of runs: reproducible from ``base_seed``, fresh entropy per invocation when it
    is None (the reference seeds nothing), and never shared between ranks or between the batches (problem shapes) of one rank."""
    if base_seed is None:
        import numpy as np
        base_seed = int(np.random.SeedSequence().entropy & 0xFFFFFFFFFFFF)
    return int(base_seed) + 7919 * int(rank) + 104729 * int(batch_index)


def my_slice(n_runs, rank=None, world=None):
    """Indices of the runs this rank owns: r = rank (mod world)."""
    if rank is None:
        rank, world, _ = dist_info()
    return list(range(rank, n_runs, world))


def gather_rows(local_rows, n_runs, rank=None, world=None, force_collective=None):
    """local_rows[len(my_slice), ...] float32 -> rows[n_runs, ...] in run order, on every rank (a single all_gather).

    force_collective (default: the environment's VAEQ_FORCE_COLLECTIVE): at world == 1 still go through the process group's
    all_gather_into_tensor on device tensors when one is initialised -- the very code N ranks execute, so RCCL (backend ``nccl``) can be
    exercised on a single GPU (tests/test_bench_gpu.py::test_rccl_gather_single_rank)."""
    if rank is None:
        rank, world, _ = dist_info()
    if force_collective is None:
        force_collective = bool(os.environ.get("VAEQ_FORCE_COLLECTIVE"))
    if world == 1 and not (force_collective and dist.is_available() and dist.is_initialized()):
        return local_rows
    per = (n_runs + world - 1) // world
    shape = (per,) + tuple(local_rows.shape[1:])
    backend = dist.get_backend()
    dev = torch.device("cuda", torch.cuda.current_device()) if backend == "nccl" else torch.device("cpu")
    buf = torch.zeros(shape, dtype=torch.float32, device=dev)
    buf[:local_rows.shape[0]] = local_rows.to(dev)
    allbuf = torch.empty((world * per,) + shape[1:], dtype=torch.float32, device=dev)   # concatenation form: nccl and gloo
    dist.all_gather_into_tensor(allbuf, buf)
    allbuf = allbuf.cpu().reshape((world,) + shape)
    out = torch.empty((n_runs,) + tuple(local_rows.shape[1:]), dtype=torch.float32)
    for k in range(world):
        out[k::world] = allbuf[k, :len(range(k, n_runs, world))]                    # run r lives on rank r % world
    return out


def run_sharded(points, shape_key, run_batch, base_seed, result_shape, row_shape, batch_offset=0, announce=True):
    """The sharded sweep of the AWGN scripts: ``points`` = [(index into the result arrays, point)], this rank's share (my_slice) run as one
    batch per problem shape -- shape_key(point), in sorted order -- and gathered once (gather_rows).

    run_batch(shape, pts, seeds, device, seed) -> rows[len(pts), *row_shape]: ``seeds`` the per-run seeds (base_seed + 1000 * the point's number,
    None without base_seed), ``seed`` = stream_seed(base_seed, rank, batch number + batch_offset), the key of the batch's device-generator streams.
    row_shape (n_eval,) gives one result array, (K, n_eval) gives K of them, each of result_shape + (n_eval,).
    Returns the list of result arrays (float32) on rank 0, None elsewhere.  announce: rank 0 prints the device line."""
    rank, world, local_rank = init_distributed()
    device = device_for_rank(local_rank, world)
    if rank == 0 and announce:
        print('Run code on: ', device, f'({world} rank(s))')
    mine = my_slice(len(points), rank, world)
    local = torch.zeros(len(mine), *row_shape, dtype=torch.float32)
    for b, shape in enumerate(sorted({shape_key(points[i][1]) for i in mine})):   # one batch per problem shape
        sel = [k for k, i in enumerate(mine) if shape_key(points[i][1]) == shape]
        local[sel] = run_batch(shape, [points[mine[k]][1] for k in sel], [None if base_seed is None else base_seed + 1000 * mine[k] for k in sel],
                               device, stream_seed(base_seed, rank, b + batch_offset))
    rows = gather_rows(local, len(points), rank, world)
    if rank != 0:
        return None
    rows = rows.reshape(len(points), *row_shape[-2:]) if len(row_shape) > 1 else rows.unsqueeze(1)
    out = [torch.empty(*result_shape, row_shape[-1], dtype=torch.float32) for _ in range(rows.shape[1])]
    for j, arr in enumerate(out):
        for k, (idx, _) in enumerate(points):
            arr[idx] = rows[k, j]
    return out


def info_rows(r, keys):
    """A runner's (SER, info) -> rows [R, 1 + len(keys), n_eval]: per run SER, then info[k] for k in keys."""
    return torch.stack([r[0]] + [r[1][k] for k in keys], dim=1)


FEC_KEYS = ("BER_post", "FER", "BER_pre_fec", "fec_iters")
FEC_OUTER_KEYS = ("BER_outer", "FER_outer")                # the two rows behind them when fec_metrics carries an outer code


def fec_keys(fec_metrics):
    """The keys a sweep script's .mat gains under its fec_metrics: none, FEC_KEYS, or FEC_KEYS + FEC_OUTER_KEYS with an outer code."""
    if fec_metrics is None:
        return ()
    return FEC_KEYS + (FEC_OUTER_KEYS if fec_metrics.get("outer") is not None else ())


def fec_values(fec):
    """fec.fec_figures' dict -> [R, 4] float32 on the CPU, in FEC_KEYS order: BER_post, FER, BER_pre and the mean over the codewords of iters;
    [R, 6] with an outer code: then BER_outer and FER_outer, in FEC_OUTER_KEYS order."""
    cols = [fec["BER_post"], fec["FER"], fec["BER_pre"], fec["iters"].double().mean(1).float()]
    if "outer" in fec:
        cols += [fec["outer"]["BER_outer"], fec["outer"]["FER_outer"]]
    return torch.stack(cols, dim=1).cpu()


def fec_rows(r, keys):
    """An AWGN runner's (SER, info or None, extras) under fec= -> rows [R, 1 + len(keys) + 4, n_eval] through info_rows: SER, info[k] for k in keys,
    then the four FEC_KEYS figures of the last evaluated validation (and the two FEC_OUTER_KEYS figures behind them with an outer code), each
    repeated along n_eval (a row has one length)."""
    v = fec_values(r[2]["fec"])
    names = (FEC_KEYS + FEC_OUTER_KEYS)[:v.shape[1]]
    cols = dict(r[1] or {}, **{k: v[:, j:j + 1].expand(-1, r[0].shape[1]) for j, k in enumerate(names)})
    return info_rows((r[0], cols), tuple(keys) + names)
