"""A/B of the device JSONL decoder (Checker.load_jsonl_many, decode="device")
against the host decoder on the C4 batch, warm, the arms alternating in one
process:

  (a) s2.load_many on 16 threads                       decode only
  (b) Checker.load_jsonl_many                          decode only, with the stage breakdown
  (c) check_jsonl_many(decode="host" | "device")       certified histories/s

and the device image of the batch compared with save_cache(load_many(blobs))
section for section. One JSON line per repetition and a summary line (median,
min, max per arm) are appended to --out.

    python tools/decode_device_ab.py [--histories 10000] [--reps 5] [--out profiles/r07/decode_device_ab.jsonl]
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def sections(img):
    """A cache image's sections (cache.cpp: magic, version, sizeof(Event), n, off[n + 1], payload)."""
    n, = struct.unpack_from("<Q", img, 16)
    off = struct.unpack_from("<%dQ" % (n + 1), img, 24)
    base = (24 + 8 * (n + 1) + 7) & ~7
    return [img[base + off[i]:base + off[i + 1]] for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--histories", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--first-seed", type=int, default=2 * 10 ** 6)  # bench.py's warm pass
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "decode_device_ab.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import s2_verification_amd as s2
    from s2_verification_amd import workloads as W

    n, reps = args.histories, max(5, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")

    def emit(d):
        line = json.dumps(d)
        out.write(line + "\n")
        out.flush()
        print(line, flush=True)

    blobs = [s2.simulate_jsonl(**W.c4_params(sd)) for sd in range(args.first_seed, args.first_seed + n)]
    jsonl_bytes = sum(map(len, blobs))
    checker = s2.Checker()
    emit({"what": "setup", "histories": n, "jsonl_bytes": jsonl_bytes, "threads": args.threads, "reps": reps,
          "chunk_mb": os.environ.get("S2LC_DEVDECODE_CHUNK_MB", "default")})

    # the device image against the CPU's, section for section (also the warm-up of both decoders)
    hs = s2.load_many(blobs, threads=args.threads)
    cpu_img = s2.save_cache(hs)
    del hs
    hs, st = checker.load_jsonl_many(blobs, threads=args.threads)
    dev_img = s2.save_cache(hs)
    del hs
    a, b = sections(cpu_img), sections(dev_img)
    differ = [i for i in range(n) if a[i] != b[i]] if len(a) == len(b) == n else [-1]
    emit({"what": "image", "sections": n, "sections_differ": len(differ), "first": differ[:5],
          "image_equal": cpu_img == dev_img, "cache_bytes": len(cpu_img), "n_device": st["n_device"],
          "n_fallback": st["n_fallback"], "n_rejected": st["n_rejected"]})
    assert not differ and cpu_img == dev_img, "the device image differs from save_cache(load_many(blobs))"
    assert st["n_rejected"] == 0
    del a, b, cpu_img, dev_img

    stages = ("stage_ms", "h2d_ms", "kernel_ms", "d2h_ms", "load_ms")
    host_ms, dev_ms, dev_st = [], [], {k: [] for k in stages}
    for rep in range(reps):
        t0 = time.perf_counter()
        hs = s2.load_many(blobs, threads=args.threads)
        t1 = time.perf_counter()
        del hs
        host_ms.append(1e3 * (t1 - t0))
        t0 = time.perf_counter()
        hs, st = checker.load_jsonl_many(blobs, threads=args.threads)
        t1 = time.perf_counter()
        del hs
        dev_ms.append(1e3 * (t1 - t0))
        for k in stages:
            dev_st[k].append(st[k])
        emit({"what": "decode", "rep": rep, "host_ms": round(host_ms[-1], 3), "device_ms": round(dev_ms[-1], 3),
              **{k: round(st[k], 3) for k in stages}, "bytes_in": st["bytes_in"], "bytes_out": st["bytes_out"],
              "n_device": st["n_device"], "n_fallback": st["n_fallback"], "n_rejected": st["n_rejected"]})
        assert st["n_rejected"] == 0 and st["n_device"] == n

    e2e = {"host": [], "device": []}
    ref = None
    for rep in range(reps + 1):  # (the first sizes the checker's two device batches: not counted)
        for mode in ("host", "device"):
            t0 = time.perf_counter()
            r = checker.check_jsonl_many(blobs, threads=args.threads, slices=2, decode=mode)
            t1 = time.perf_counter()
            wl = np.diff(r["witness_offs"].astype(np.int64))
            bad = int(np.sum((r["verdict"] == s2.S2LC_OK) & (wl == 0)))
            assert bad == 0, "an Ok without a certified witness"
            if ref is None:
                ref = r
            same = all(np.array_equal(r[k], ref[k]) for k in ("verdict", "witness_offs", "witness_ids"))
            assert same, "the arms disagree"
            if rep:
                e2e[mode].append(n / (t1 - t0))
                emit({"what": "e2e", "rep": rep - 1, "decode": mode, "histories_per_sec": round(n / (t1 - t0), 1),
                      "seconds": round(t1 - t0, 4), "ok": int(np.sum(r["verdict"] == s2.S2LC_OK)),
                      "ok_without_witness": bad})
            del r

    km, hm = statistics.median(dev_st["kernel_ms"]), statistics.median(dev_st["h2d_ms"])
    emit({"what": "summary", "histories": n, "jsonl_bytes": jsonl_bytes,
          "decode_host_ms": spread(host_ms), "decode_device_ms": spread(dev_ms),
          **{"device_" + k: spread(dev_st[k]) for k in stages},
          "kernel_lt_h2d": bool(km < hm), "kernel_text_GBps": round(jsonl_bytes / km / 1e6, 1),
          "h2d_GBps": round(jsonl_bytes / hm / 1e6, 1),
          "e2e_host_hps": spread(e2e["host"]), "e2e_device_hps": spread(e2e["device"]),
          "e2e_device_over_host": round(statistics.median(e2e["device"]) / statistics.median(e2e["host"]), 3)})
    return 0


if __name__ == "__main__":
    sys.exit(main())
