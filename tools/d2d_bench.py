#!/usr/bin/env python3
"""What the device-resident container costs, measured in one process:

  container   1 GiB in 4 MiB blocks, generated on the device (splitmix64 bytes and Zipf text):
              bmh_compress_d2d against bmh_encode_blocks_dev and bmh_decompress_d2d against
              bmh_decode_blocks_dev on the same data, alternating, host clock around the
              (synchronous) calls. The difference is the container: tables, the record copy, CRCs.
  gather      a 256 MiB container of 4 MiB blocks read back by bmh_readv_d2d as one 256 MiB range
              and as 65 536 ranges of 4 KiB (shuffled): the gather_pieces kernel time from the
              context's kernel timing, against hipMemcpyAsync device-to-device of the same bytes
              (one copy between two events; 65 536 copies under a host clock to the synchronise).

Every shape is warmed up before it is timed. Writes one JSON document. Needs a gfx950 GPU: it
fails without one.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bwt-mtf-huffman-compressor_amd"))
import bmh  # noqa: E402

D2D = 3  # hipMemcpyDeviceToDevice


def stat(v):
    v = np.asarray(v, dtype=np.float64)
    return {"mean": float(v.mean()), "min": float(v.min()), "max": float(v.max()), "runs": len(v)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def container_cost(ctx, n, bs, reps, kind):
    offs = np.minimum(np.arange(0, n + bs, bs, dtype=np.uint64), np.uint64(n))
    cap = int(bmh.lib().bmh_compress_bound_checked(n, bs))
    d_in, d_rec, d_box, d_out = ctx.alloc(n), ctx.alloc(cap), ctx.alloc(cap), ctx.alloc(n)
    (ctx.synth_zipf(d_in, n) if kind == "text" else ctx.synth_splitmix64(d_in, n, seed=0))
    t = {k: [] for k in ("encode_blocks_dev", "compress_d2d", "compress_d2d_checksum", "decode_blocks_dev",
                         "decompress_d2d", "decompress_d2d_checksum", "verify_d2d_checksum")}
    for rep in range(-2, reps):  # two warm-up rounds of every shape
        keep = rep >= 0
        r = {}
        r["encode_blocks_dev"] = timed(lambda: r.update(ro=ctx.encode_blocks_dev(d_in, offs, d_rec, cap)))
        r["compress_d2d"] = timed(lambda: r.update(l1=ctx.compress_d2d(d_in, n, bs, d_box, cap)))
        r["decode_blocks_dev"] = timed(lambda: ctx.decode_blocks_dev(d_rec, r["ro"], d_out, n))
        r["decompress_d2d"] = timed(lambda: ctx.decompress_d2d(d_box, r["l1"], d_out, n))
        r["compress_d2d_checksum"] = timed(lambda: r.update(l2=ctx.compress_d2d(d_in, n, bs, d_box, cap, checksum=True)))
        r["decompress_d2d_checksum"] = timed(lambda: ctx.decompress_d2d(d_box, r["l2"], d_out, n))
        r["verify_d2d_checksum"] = timed(lambda: ctx.verify_d2d(d_box, r["l2"]))
        if keep:
            for k in t:
                t[k].append(r[k])
    out = {"bytes": n, "block": bs, "kind": kind, "records_bytes": int(r["ro"][-1]), "container_bytes": int(r["l1"]),
           "ms": {k: stat(v) for k, v in t.items()},
           "gb_per_s_mean": {k: n / (np.mean(v) * 1e-3) / 1e9 for k, v in t.items()}}
    for d in (d_in, d_rec, d_box, d_out):
        d.free()
    return out


class Hip:
    def __init__(self):
        self.l = C.CDLL("libamdhip64.so")
        self.l.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.l.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.l.hipEventSynchronize.argtypes = [C.c_void_p]
        self.l.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        self.l.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.a, self.b = C.c_void_p(), C.c_void_p()
        self.ok(self.l.hipEventCreate(C.byref(self.a)))
        self.ok(self.l.hipEventCreate(C.byref(self.b)))

    @staticmethod
    def ok(e):
        if e != 0:
            raise RuntimeError(f"HIP error {e}")

    def copy_ms(self, stream, dst, src, n):
        """One device-to-device copy between two events."""
        self.ok(self.l.hipEventRecord(self.a, stream))
        self.ok(self.l.hipMemcpyAsync(dst, src, n, D2D, stream))
        self.ok(self.l.hipEventRecord(self.b, stream))
        self.ok(self.l.hipEventSynchronize(self.b))
        ms = C.c_float()
        self.ok(self.l.hipEventElapsedTime(C.byref(ms), self.a, self.b))
        return ms.value

    def copies_ms(self, stream, dst, src, offs_dst, offs_src, n):
        """One copy per piece, host clock up to the synchronise (what the caller would wait)."""
        t0 = time.perf_counter()
        f = self.l.hipMemcpyAsync
        for od, os_ in zip(offs_dst, offs_src):
            f(dst + od, src + os_, n, D2D, stream)
        self.ok(self.l.hipStreamSynchronize(stream))
        return (time.perf_counter() - t0) * 1e3


def gather_cost(ctx, n, bs, reps):
    cap = int(bmh.lib().bmh_compress_bound(n, bs))
    d_in, d_box, d_out = ctx.alloc(n), ctx.alloc(cap), ctx.alloc(n)
    ctx.synth_zipf(d_in, n)
    length = ctx.compress_d2d(d_in, n, bs, d_box, cap)
    piece = 4096
    src = np.random.default_rng(5).permutation(n // piece).astype(np.uint64) * np.uint64(piece)
    shapes = {"one_range": ([0], [n]), "ranges_4k": (src, np.full(src.size, piece, np.uint64))}
    hip = Hip()
    stream = lib_stream(ctx)
    res = {"bytes": n, "block": bs}
    ctx.set_timing(True)
    for name, (o, k) in shapes.items():
        kern, call = [], []
        for rep in range(-2, reps):
            ctx.reset_stats()
            ms = timed(lambda: ctx.readv_d2d(d_box, length, o, k, d_out, n))
            st = ctx.kernel_stats()
            if rep >= 0:
                call.append(ms)
                kern.append(st["gather_pieces"][1])
        res[name] = {"gather_pieces_kernel_ms": stat(kern), "gather_pieces_gb_per_s": n / (np.mean(kern) * 1e-3) / 1e9,
                     "readv_call_ms_timing_on": stat(call), "gather_launches_per_call": st["gather_pieces"][0]}
    ctx.set_timing(False)
    got = d_out.download(1 << 20, n - (1 << 20))  # the shuffled read did land the bytes
    assert np.array_equal(got[:piece], d_in.download(piece, int(src[-256])))
    a, b = d_in.ptr.value, d_out.ptr.value
    one = [hip.copy_ms(stream, b, a, n) for _ in range(reps + 2)][2:]
    dst = (np.arange(src.size, dtype=np.uint64) * np.uint64(piece)).tolist()
    many = [hip.copies_ms(stream, b, a, dst, src.tolist(), piece) for _ in range(3)][1:]
    res["one_range"]["hipMemcpyAsync_ms"] = stat(one)
    res["one_range"]["hipMemcpyAsync_gb_per_s"] = n / (np.mean(one) * 1e-3) / 1e9
    res["ranges_4k"]["hipMemcpyAsync_each_ms_host_clock"] = stat(many)
    for d in (d_in, d_box, d_out):
        d.free()
    return res


def lib_stream(ctx):
    return C.c_void_p(bmh.lib().bmh_ctx_stream(ctx.h))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--block", type=int, default=4 << 20)
    ap.add_argument("--gather-bytes", type=int, default=256 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "d2d_bench.json"))
    a = ap.parse_args()
    res = {"reps": a.reps}
    with bmh.Context(0) as ctx:
        res["gather"] = gather_cost(ctx, a.gather_bytes, a.block, a.reps)
        res["container"] = [container_cost(ctx, a.bytes, a.block, a.reps, kind) for kind in ("random", "text")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
