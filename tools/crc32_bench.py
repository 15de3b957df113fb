#!/usr/bin/env python3
"""Cost of the CRC-32 integrity check (DESIGN "Integrity"), measured in one process:

  kernel      1 GiB of device-generated splitmix64 bytes in 4 MiB blocks; after a warm-up, 20
              bmh_crc32_dev calls with the context's kernel timing on: the summed crc32_* kernel
              time per call, against mtf_hist (the project's one-pass streaming read) timed the
              same way on the same bytes, and against the read floor (1 GiB over peak HBM rate).
  end to end  bmh_compress_host on page-locked buffers with BMH_OPT_CHECKSUM off and on,
              alternating, five pairs: both means and the spread of the off runs.

Writes one JSON document (default profiles/r07/crc32_v1.json). Needs a gfx950 GPU: it fails
without one.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bwt-mtf-huffman-compressor_amd"))
import bmh  # noqa: E402

HBM_PEAK_SPEC = 8.0e12      # bytes/s, datasheet
HBM_PEAK_MEASURED = 6.29e12  # bytes/s, float4 copy


def kernel_ms(ctx, names):
    st = ctx.kernel_stats()
    return {k: st[k][1] for k in st if any(k.startswith(n) for n in names)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--block", type=int, default=4 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=5, help="end-to-end off/on pairs (0: kernels only, writes no file)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r07", "crc32_v1.json"))
    a = ap.parse_args()
    n, bs = a.bytes, a.block
    offs = np.minimum(np.arange(0, n + bs, bs, dtype=np.uint64), np.uint64(n))
    nb = len(offs) - 1
    res = {"bytes": n, "block": bs, "blocks": nb, "calls": a.calls}
    with bmh.Context(0) as ctx:
        d_in, d_mtf = ctx.alloc(n), ctx.alloc(n)
        ctx.synth_splitmix64(d_in, n, seed=0)
        # ---- kernel cost: crc32_* and mtf_hist, same process, same bytes
        for _ in range(3):
            crc = ctx.crc32_dev(d_in, offs)
        ctx.mtf_dev(d_in, offs, d_mtf)
        ctx.set_timing(True)
        per_call, wall = [], []
        for _ in range(a.calls):
            ctx.reset_stats()
            t0 = time.perf_counter()
            ctx.crc32_dev(d_in, offs)
            wall.append((time.perf_counter() - t0) * 1e3)
            per_call.append(kernel_ms(ctx, ["crc32_"]))
        hist = []
        for _ in range(a.calls):
            ctx.reset_stats()
            ctx.mtf_dev(d_in, offs, d_mtf)
            hist.append(kernel_ms(ctx, ["mtf_hist"])["mtf_hist"])
        # the same read over the MTF stage's output bytes, for a like-for-like histogram input
        crc_mtf = []
        for _ in range(a.calls):
            ctx.reset_stats()
            ctx.crc32_dev(d_mtf, offs)
            crc_mtf.append(sum(kernel_ms(ctx, ["crc32_"]).values()))
        ctx.set_timing(False)
        tiles = np.array([c["crc32_tiles"] for c in per_call])
        fold = np.array([c["crc32_fold"] for c in per_call])
        tot = tiles + fold
        scale = (1 << 30) / n
        res["kernel"] = {
            "crc32_tiles_ms_mean": float(tiles.mean()), "crc32_fold_ms_mean": float(fold.mean()),
            "crc32_ms_per_call": {"mean": float(tot.mean()), "min": float(tot.min()), "max": float(tot.max())},
            "crc32_ms_per_gib": float(tot.mean() * scale),
            "crc32_on_mtf_bytes_ms_mean": float(np.mean(crc_mtf)),
            "crc32_dev_wall_ms_mean": float(np.mean(wall)),
            "mtf_hist_ms_per_call": {"mean": float(np.mean(hist)), "min": float(np.min(hist)), "max": float(np.max(hist))},
            "ratio_to_mtf_hist": float(tot.mean() / np.mean(hist)),
            "target_ratio": 2.0,
            "read_floor_ms": {"spec_8.0TBps": n / HBM_PEAK_SPEC * 1e3, "measured_6.29TBps": n / HBM_PEAK_MEASURED * 1e3},
            "achieved_TBps": float(n / (tot.mean() * 1e-3) / 1e12),
            "share_of_measured_read_floor": float(n / HBM_PEAK_MEASURED * 1e3 / tot.mean()),
            "crc_of_block0": int(crc[0]),
        }
        if a.pairs == 0:  # kernels only (a profiler run)
            d_in.free()
            d_mtf.free()
            print(json.dumps(res))
            return
        # ---- end to end: pinned in / out, option off and on alternating in this process
        cap = int(bmh.lib().bmh_compress_bound_checked(n, bs))
        hin, hout = ctx.alloc_host(n), ctx.alloc_host(cap)
        step = 256 << 20
        for o in range(0, n, step):
            hin.a[o:o + step] = d_in.download(min(step, n - o), o)
        d_in.free()
        d_mtf.free()
        times = {0: [], 1: []}
        sizes = {}
        try:
            for v in (0, 1):  # warm-up of both shapes
                ctx.set_option("checksum", v)
                ctx.compress_into(hin.a, bs, hout.a)
            for _ in range(a.pairs):
                for v in (0, 1):
                    ctx.set_option("checksum", v)
                    t0 = time.perf_counter()
                    sizes[v] = ctx.compress_into(hin.a, bs, hout.a)
                    times[v].append((time.perf_counter() - t0) * 1e3)
        finally:
            ctx.set_option("checksum", 0)
        res["end_to_end"] = {
            "off_ms": times[0], "on_ms": times[1], "off_mean_ms": float(np.mean(times[0])),
            "on_mean_ms": float(np.mean(times[1])), "off_spread_ms": float(max(times[0]) - min(times[0])),
            "on_minus_off_ms": float(np.mean(times[1]) - np.mean(times[0])),
            "out_bytes_off": sizes[0], "out_bytes_on": sizes[1],
        }
        hin.free()
        hout.free()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
