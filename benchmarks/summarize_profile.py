"""gpurun_out/prof_<tag>/ (written by benchmarks/profile.sh) -> profiles/<tag>_kernel_stats.csv and
profiles/<tag>_pmc_summary.json (per-launch averages of the scan kernel, HBM traffic with the gfx950
FETCH_SIZE correction of MI355X_MICROARCH.md)."""
import collections, csv, glob, json, os, shutil, sys
tag = sys.argv[1]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
base = os.path.join(root, "gpurun_out", "prof_" + tag)
alg = int(sys.argv[2]) if len(sys.argv) > 2 else 2 ** 30
# the headline instance: the lean one (no equal-n-gram sets, bands for k <= 2), hash windows (NWIN = 2, DH = 3), low-bits slot
HEAD_KERNEL = "fz_lean_scan_kernel<2, 3, true>"
TILES_PER_WG = 12
# threads of the headline launch: round 1-2 (and inputs of 10+ rounds): one workgroup per 12 tiles; round 3: a whole
# number of rounds of the 6 x 256 resident workgroups, ~9.5 tiles each (fzhip.hip: enqueue_shard)
_tiles, _resident = alg // 16384, 256 * 6
HEAD_GRIDS = {(_tiles // TILES_PER_WG) * 256, max(1, (2 * _tiles + _resident * 19 // 2) // (_resident * 19)) * _resident * 256}
newest = lambda pattern: max(glob.glob(pattern), key=os.path.getmtime)   # gpurun merges runs: take the last one
stats = newest(os.path.join(base, "stats", "*", "*_kernel_stats.csv"))
shutil.copy(stats, os.path.join(root, "profiles", tag + "_rocprof_kernel_stats.csv"))
# rocprofv3's own --stats table covered only the last few dispatches of the run (12 of 510 here), so the
# per-kernel table that is committed is rebuilt from the full --kernel-trace of the same run
trace = newest(os.path.join(base, "stats", "*", "*_kernel_trace.csv"))
per = collections.defaultdict(list)
head = []                              # the headline launches: the 3-block DNA kernel over 1 GiB (4096 workgroups)
for r in csv.DictReader(open(trace)):
    dur = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    name = r["Kernel_Name"]
    grid = int(r.get("Grid_Size_X", r.get("Grid_Size", "0")) or 0)
    if HEAD_KERNEL in name:
        name += " [grid %d]" % grid
        if grid in HEAD_GRIDS:
            head.append(dur)
    per[name].append(dur)
total = sum(sum(v) for v in per.values())
with open(os.path.join(root, "profiles", tag + "_kernel_stats.csv"), "w", newline="") as f:
    wr = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
    wr.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs", "MedianNs"])
    for name, v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        vs = sorted(v)
        wr.writerow([name, len(v), sum(v), round(sum(v) / len(v), 1), round(100.0 * sum(v) / total, 2), vs[0], vs[-1], vs[len(vs) // 2]])
avg_ns, kname, calls = sum(head) / len(head), "void " + HEAD_KERNEL, len(head)
out = {}
for d in sorted(glob.glob(os.path.join(base, "pmc*"))):
    if not os.path.isdir(d):
        continue
    f = newest(os.path.join(d, "*", "*_counter_collection.csv"))
    agg = collections.defaultdict(list)
    for r in csv.DictReader(open(f)):
        if HEAD_KERNEL in r["Kernel_Name"]:
            agg[r["Counter_Name"]].append(float(r["Counter_Value"]))
    for k, v in agg.items():
        out[k] = sum(v) / len(v)
fetch_raw = out["FETCH_SIZE"] * 1024
traffic = fetch_raw * 2 + out["WRITE_SIZE"] * 1024
summary = {
    "command": "benchmarks/profile.sh %s: rocprofv3 --kernel-trace --stats, then 4 separate rocprofv3 --pmc passes, each around "
               "`python bench.py --steps 10 --warmup 2 --no-cpu-baseline`" % tag,
    "kernel": kname.split("(")[0],
    "kernel_trace_avg_ns": avg_ns, "kernel_trace_calls": calls,
    "algorithmic_bytes_per_launch": alg,
    "counters_per_launch": out,
    "hbm_traffic": {
        "FETCH_SIZE_raw_bytes": fetch_raw,
        "gfx950_correction": "x2: FETCH_SIZE tallies 128-B requests at 64 B on gfx950 for wide coalesced streaming reads "
                             "(MI355X_MICROARCH.md, HBM section)",
        "fetch_bytes_corrected": fetch_raw * 2, "write_bytes": out["WRITE_SIZE"] * 1024,
        "traffic_bytes": traffic, "traffic_over_algorithmic": traffic / alg,
        "note": "candidate windows are requested by LDS-DMA right after the tile that produced the hit (round 2); round 1 "
                "fetched them when a wave's queue was flushed, long after those tiles had left L2: 1.11 x the "
                "algorithmic bytes",
    },
    "derived": {
        "valu_ops_per_sequence_byte": out["SQ_INSTS_VALU"] * 64 / alg,
        "salu_ops_per_sequence_byte_x64": out["SQ_INSTS_SALU"] * 64 / alg,
        "wave_cycle_split": {k: out[c] / out["SQ_WAVE_CYCLES"] for k, c in
                             (("active", "SQ_ACTIVE_INST_ANY"), ("wait_any", "SQ_WAIT_ANY"), ("wait_inst_any", "SQ_WAIT_INST_ANY"))},
        "achieved_GBps_kernel_trace": alg / (avg_ns * 1e-9) / 1e9,
    },
}
json.dump(summary, open(os.path.join(root, "profiles", tag + "_pmc_summary.json"), "w"), indent=1)
print(json.dumps({k: summary[k] for k in ("kernel", "kernel_trace_avg_ns", "hbm_traffic", "derived")}, indent=1))
