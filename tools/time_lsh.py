#!/usr/bin/env python3
"""The exhaustive Hamming scan (vlq.GpuLSH.search_codes, csrc/scan_hamming.hip) over the shapes csrc/hamming_plan.h has to decide:

    nq in {1, 64, 10000}   ntotal in {1e5, 1e6, 1e7}   code size in {8, 32, 128} bytes   k in {10, 100, 1024}

Random codes and query codes, device-resident; every call is timed with events on the stream the index uses.  Before anything is
timed the device is kept busy for about a second (clocks), every variant of a shape runs untimed first, the variants alternate
inside every repetition, and a row reports the median and the minimum / maximum over the repetitions.  Variants: the plan's own
choice; the query tile forced to Q = 1, 2, 4 (slices left to the plan); for the small batches the slices forced to 8, 16, 32, 64
(tile left to the plan) -- the comparisons that fix kHamTile, kHamTargetGroups and kHamMinSlice.  All variants of a shape must
give identical rows; the tool refuses to report a shape where they do not.

Every row is set against two floors computed from the shape (MI355X_MICROARCH.md: 6.29 TB/s measured HBM rate; 256 CUs x 4 SIMDs
x 32 lanes per clock at 2.4 GHz = 78.6e12 vector lane-operations per second):
    stream_ms   ntotal * code_size * ceil(nq / Q) bytes of codes, whatever S is, at the HBM rate (a repeated pass over a code set
                that fits the caches is served faster than this: the floor is then not a floor, and the row says so by beating it)
    issue_ms    nq * ntotal * (code_size / 4) words, one XOR and one popcount-accumulate each

    python tools/time_lsh.py [reps] [out.json] [quick]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import vector_line_quantization_amd as vlq

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
out_file = sys.argv[2] if len(sys.argv) > 2 else None
quick = len(sys.argv) > 3 and sys.argv[3] == "quick"
if not torch.cuda.is_available():
    raise SystemExit("tools/time_lsh.py needs a HIP device: nothing here is measured on a CPU")
dev = torch.device("cuda", 0)
HBM, LANE_OPS = 6.29e12, 256 * 4 * 32 * 2.4e9
NQS, NTS, CSS, KS = (1, 64, 10000), (100000, 1000000, 10000000), (8, 32, 128), (10, 100, 1024)
if quick:
    NTS = (100000, 1000000)
torch.manual_seed(5)
stream = torch.cuda.current_stream()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


rows = []
warmed = False
for cs in CSS:
    for nt in NTS:
        g = vlq.GpuLSH(cs * 8, cs * 8, rotate_data=False)
        g.set_stream(stream.cuda_stream)
        codes = torch.randint(0, 256, (nt, cs), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        g.add_codes(codes)
        torch.cuda.synchronize()
        del codes
        q_all = torch.randint(0, 256, (max(NQS), cs), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        if not warmed:
            D = torch.empty((1000, 10), dtype=torch.float32, device=dev)
            I = torch.empty((1000, 10), dtype=torch.int64, device=dev)
            t_end = time.time() + 1.0
            while time.time() < t_end:          # clocks up before the first timed call
                g.search_codes(q_all[:1000], 10, D, I)
                torch.cuda.synchronize()
            warmed = True
        for nq in NQS:
            for k in KS:
                q = q_all[:nq].contiguous()
                names = ["plan", "q1"] + ([] if k > 256 else ["q2", "q4"]) + (["s8", "s16", "s32", "s64"] if nq <= 64 else [])
                D = {n: torch.empty((nq, k), dtype=torch.float32, device=dev) for n in names}
                I = {n: torch.empty((nq, k), dtype=torch.int64, device=dev) for n in names}

                def new(name):
                    qt = int(name[1:]) if name[0] == "q" else 0
                    s = int(name[1:]) if name[0] == "s" else 0

                    def run():
                        g.scan_split(qt, s)
                        g.search_codes(q, k, D[name], I[name])
                    return run
                variants = {n: new(n) for n in names}
                info = {}
                for name, fn in variants.items():       # untimed: code objects, workspaces
                    fn(); fn()
                    info[name] = g.last_scan_info()       # (synchronises)
                ms = {n: [] for n in variants}
                for _ in range(reps):
                    for name, fn in variants.items():
                        ms[name].append(timed(fn))
                torch.cuda.synchronize()
                if not all(torch.equal(D[n], D["plan"]) and torch.equal(I[n], I["plan"]) for n in names):
                    raise SystemExit("cs %d ntotal %d nq %d k %d: the variants' rows differ" % (cs, nt, nq, k))
                Q = int(info["plan"].split("Q=")[1].split()[0])
                row = {"code_size": cs, "ntotal": nt, "nq": nq, "k": k, "scan": info,
                       "stream_ms": 1e3 * nt * cs * ((nq + Q - 1) // Q) / HBM, "issue_ms": 1e3 * nq * nt * (cs // 4) * 2 / LANE_OPS}
                for name in ms:
                    row[name] = {"median_ms": statistics.median(ms[name]), "min_ms": min(ms[name]), "max_ms": max(ms[name])}
                rows.append(row)
                print("cs %3d nt %8d nq %5d k %4d  plan %9.3f ms [%8.3f .. %8.3f]  floors: stream %9.3f issue %9.3f  | %s | %s"
                      % (cs, nt, nq, k, row["plan"]["median_ms"], row["plan"]["min_ms"], row["plan"]["max_ms"], row["stream_ms"], row["issue_ms"],
                         " ".join("%s %.3f" % (n, row[n]["median_ms"]) for n in names[1:]), info["plan"]), flush=True)
        g.close()
        del q_all
result = {"reps": reps, "device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM, "lane_ops_per_s": LANE_OPS, "rows": rows}
if out_file:
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    with open(out_file, "w") as f:
        json.dump(result, f, indent=1)
