#!/usr/bin/env python3
"""Time vaeq_chase_decode (GPU), the Chase-decoded inner code, at the size of a sweep and look at what it leaves the staircase code: --runs runs x
the 937 words of hamming_code(7), the extended (128, 120) code, that fit the 120 000 bits of a 10 000-symbol DP 64-QAM frame (w = 12 planes), with
0, 4 and 6 test-pattern positions, at three synthetic pre-FEC error rates.

    python tools/probe_chase.py [--runs 8192] [--symbols 10000] [--bers 0.005,0.0125,0.02] [--patterns 0,4,6] [--rounds 5] [--out profiles/chase/probe.txt]

--out is written anew by every run; the committed file is the run with the defaults.

The LLRs are synthetic BPSK + AWGN LLRs generated on the device from a seed: random TX bits, y = (1 - 2 b) + sigma noise with sigma chosen so that
Q(1 / sigma) is the level's bit error rate, llr = 2 y / sigma^2.  Per (level, patterns), after a warm-up call, --rounds calls between device events
(host wrapper + kernel): median / min / max, once with the payload stream (the call the concatenation makes) and once without.  Beside every line
the floor of reading llr and bits once, 5 R w N bytes, at the copy bandwidth measured in the same session with bench.py's stream_copy_gbs
(vaeq_stream_copy: read + write bytes per second of a plain 16-byte grid-stride copy); the bytes of the stream the call also writes; the inner
decoder's figures; and BER_post and the mean errors per block (pos_err) of StaircaseCode(BchCode(8, 3, n=240), 7) at window 4 behind the inner code
-- one chain in the run's 937 x 120 payload bits, bit-interleaved -- and alone on the same LLRs.  One JSON line per (level, patterns)."""
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
from tools.probe_staircase import timed  # noqa: E402


def staircase_figures(res):
    return dict(BER_post=float(res["BER_post"].double().mean()), errors_in=round(float(res["pre_err"].double().mean()), 2),
                ok_share=round(float(res["ok"].double().mean()), 4), pos_err=[round(float(x), 3) for x in res["pos_err"].double().mean((0, 1))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=8192)
    ap.add_argument("--symbols", type=int, default=10000)
    ap.add_argument("--bers", default="0.005,0.0125,0.02")
    ap.add_argument("--patterns", default="0,4,6")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chase", "probe.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    w, R, N = 12, a.runs, a.symbols
    code = engine.hamming_code(7)
    C_ = N * w // code.n
    stair = engine.StaircaseCode(engine.BchCode(8, 3, n=240), 7)
    copy_gbs = bench.stream_copy_gbs(dev)
    floor_ms = 5 * R * w * N / (copy_gbs * 1e9) * 1e3
    stream_gb = 5 * R * C_ * code.k / 1e9
    lines = [f"# vaeq_chase_decode: {R} runs x {C_} words of the extended Hamming code ({code.n}, {code.k}), r = {code.r}, w = {w}, {N} symbols, "
             f"bit-packed map, payload {code.k}, spread; behind it StaircaseCode(BchCode(8, 3, n=240), {stair.L}), n_chain = {stair.n}, window "
             f"{a.window}, at most {a.iters} iterations per position, {C_ * code.k // stair.n} chain in the {C_ * code.k} stream bits; "
             f"{torch.cuda.get_device_name(dev)}",
             f"# copy bandwidth (vaeq_stream_copy, read + write): {copy_gbs:.0f} GB/s; llr and bits once: 5 x {R} x {w} x {N} B = "
             f"{5 * R * w * N / 1e9:.3f} GB -> floor {floor_ms:.3f} ms; the stream the call also writes: {stream_gb:.3f} GB"]
    print("\n".join(lines), flush=True)
    llr = torch.empty(R, w, N, dtype=torch.float32, device=dev)
    for k, ber in enumerate(float(x) for x in a.bers.split(",")):
        sigma = 1.0 / statistics.NormalDist().inv_cdf(1.0 - ber)
        g.manual_seed(1 + k)
        bits = torch.randint(0, 2, llr.shape, dtype=torch.int8, device=dev, generator=g)
        llr.normal_(0.0, sigma, generator=g)
        llr.add_(1.0 - 2.0 * bits.float()).mul_(2.0 / sigma ** 2)
        alone = staircase_figures(engine.staircase_decode(llr, bits, stair, a.window, chains=1, iters=a.iters, want_profile=True))
        for p in (int(x) for x in a.patterns.split(",")):
            res = engine.chase_decode(llr, bits, code, patterns=p, want_stream=True)
            behind = staircase_figures(engine.staircase_decode(res["stream"]["llr"], res["stream"]["bits"], stair, a.window, iters=a.iters,
                                                               want_profile=True))
            torch.cuda.synchronize()
            status = torch.stack([(res["status"] == s).double().mean() for s in range(3)]).tolist()
            fig = dict(BER_pre=float(res["BER_pre"].double().mean()), BER_post=float(res["BER_post"].double().mean()),
                       BER_payload=float(res["BER_payload"].double().mean()), FER=float(res["FER"].double().mean()),
                       status_share=[round(x, 4) for x in status], miscorrected_per_run=float(res["miscorrected"].double().mean()))
            del res
            t = timed(lambda: engine.chase_decode(llr, bits, code, patterns=p, want_stream=True), a.rounds)
            t0 = timed(lambda: engine.chase_decode(llr, bits, code, patterns=p), a.rounds)
            line = json.dumps(dict(ber=ber, sigma=round(sigma, 5), patterns=p, words=R * C_, **t, floor_ms=round(floor_ms, 3),
                                   floor_share=round(floor_ms / t["median_ms"], 4), no_stream_median_ms=t0["median_ms"],
                                   no_stream_min_ms=t0["min_ms"], no_stream_max_ms=t0["max_ms"],
                                   no_stream_floor_share=round(floor_ms / t0["median_ms"], 4),
                                   Mwords_per_s=round(R * C_ / t["median_ms"] / 1e3, 1), **fig, staircase_behind=behind, staircase_alone=alone))
            print(line, flush=True)
            lines.append(line)
        del bits
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
