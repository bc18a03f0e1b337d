#!/usr/bin/env python3
"""Time vaeq_bch_outer (GPU) at the size of a sweep, behind the LDPC decoder of tools/probe_ldpc.py: --runs runs x the 23 codewords of one
10 000-symbol DP 64-QAM frame (w = 12 planes) under array_code(4, 24, 211) (n = 5064, payload K = 4220), at three noise levels, with
BchCode(13, 12) behind it: n_o = 8191, C_o = 23 x 4220 // 8191 = 11 outer codewords per run.

    python tools/probe_bch.py [--runs 8192] [--symbols 10000] [--sigmas 0.3,0.53,0.8] [--rounds 5] [--out profiles/bch_outer/probe.txt]

Per level: the float32 LDPC call (engine.ldpc_decode, want_post) on tools/probe_ldpc.py's synthetic tensors, timed before and after the outer
calls in the same session -- the yardstick that shows the box's drift -- and engine.bch_outer on its `post` with the spread on and off.  After a
warm-up call, --rounds calls between device events (host wrapper + kernel): median / min / max.  Beside every outer line the floor of reading
the payload once -- R C K values of `post` (4 bytes) and of `bits` (1 byte) -- at the copy bandwidth measured in the same session with bench.py's
stream_copy_gbs (vaeq_stream_copy: read + write bytes per second of a plain 16-byte grid-stride copy), and the figures the call returns.
One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from vae_equalizer_amd import engine  # noqa: E402


def timed(f, rounds):
    f()                                                        # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return dict(median=round(statistics.median(times), 3), min=round(min(times), 3), max=round(max(times), 3), rounds=rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8192)
    ap.add_argument("--symbols", type=int, default=10000)
    ap.add_argument("--sigmas", default="0.3,0.53,0.8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bch_outer", "probe.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    code, outer, w, R, N = engine.array_code(4, 24, 211), engine.BchCode(13, 12), 12, a.runs, a.symbols
    K, C_ = (code.nb - code.mb) * code.Z, N * w // code.n
    C_o = C_ * K // outer.n
    copy_gbs = bench.stream_copy_gbs(dev)
    payload_bytes = R * C_ * K * 5
    floor_ms = payload_bytes / (copy_gbs * 1e9) * 1e3
    lines = [f"# vaeq_bch_outer behind vaeq_ldpc_decode: {R} runs x {C_} codewords of array_code(4, 24, 211), n = {code.n}, payload K = {K}, w = {w}, "
             f"{N} symbols, max_iter {a.max_iter}; BchCode(13, 12): n_o = {outer.n}, parity {outer.parity}, C_o = {C_o} per run, "
             f"{R * C_o} outer codewords; {torch.cuda.get_device_name(dev)}",
             f"# copy bandwidth (vaeq_stream_copy, read + write): {copy_gbs:.0f} GB/s; the payload once: {R} x {C_} x {K} x (4 + 1) B = "
             f"{payload_bytes / 1e9:.3f} GB -> floor {floor_ms:.3f} ms"]
    print("\n".join(lines), flush=True)
    llr = torch.empty(R, w, N, dtype=torch.float32, device=dev)

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        lines.append(line)

    for k, sigma in enumerate(float(s) for s in a.sigmas.split(",")):
        g.manual_seed(1 + k)
        bits = torch.randint(0, 2, llr.shape, dtype=torch.int8, device=dev, generator=g)
        llr.normal_(generator=g).mul_(sigma).add_(1.0).sub_(bits, alpha=2.0).mul_(2.0 / sigma ** 2)
        ldpc = lambda: engine.ldpc_decode(llr, bits, code, max_iter=a.max_iter)  # noqa: E731
        emit(dict(sigma=sigma, call="vaeq_ldpc_decode, before", unit="ms per call (host wrapper + kernel, device events)", **timed(ldpc, a.rounds)))
        res = engine.ldpc_decode(llr, bits, code, max_iter=a.max_iter, want_post=True)
        post = res["post"]
        for spread in (True, False):
            f = lambda: engine.bch_outer(post, bits, outer, code.n, payload=K, spread=spread)  # noqa: E731
            t = timed(f, a.rounds)
            o = f()
            emit(dict(sigma=sigma, call=f"vaeq_bch_outer, spread {'on' if spread else 'off'}", unit="ms per call (host wrapper + kernel, device events)", **t,
                      outer_codewords_per_s=round(R * C_o / t["median"] * 1e3), payload_GB_per_s=round(payload_bytes / t["median"] / 1e6, 1),
                      floor_ms=round(floor_ms, 3), share_of_floor=round(floor_ms / t["median"], 4),
                      status=[int((o["status"] == s).sum()) for s in range(3)], BER_post=float(res["BER_post"].double().mean()),
                      FER=float(res["FER"].double().mean()), BER_in=float(o["BER_in"].double().mean()),
                      BER_outer=float(o["BER_outer"].double().mean()), FER_outer=float(o["FER_outer"].double().mean()),
                      runs_clean_after_outer=int((o["BER_outer"] == 0).sum()), miscorrected=int(o["miscorrected"].sum()),
                      undetected=int(o["undetected"].sum())))
            del o
        del post, res
        emit(dict(sigma=sigma, call="vaeq_ldpc_decode, after", unit="ms per call (host wrapper + kernel, device events)", **timed(ldpc, a.rounds)))
        del bits
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
