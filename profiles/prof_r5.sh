#!/bin/bash
# Round-5 profile of a bench run: kernel times from a --kernel-trace --stats pass, counters from counters-only --pmc passes
# (separate runs, the program directly after --).  Every pass under its own time limit, chained: a pass that fails ends the script.
# usage: profiles/prof_r5.sh <tag> <git rev of the tree> [bench args, e.g. --exact]   -> bench_out/prof_r5_<tag>/summary.json (PROF_OUT=dir: under dir)
# Run from the root of the tree to profile (its bench.py and its library); environment knobs (RTM_DEBUG_ZERO_SKIP ...) pass through.
set -o pipefail
R=$(pwd); TAG=${1:-tolerance}; REV=${2:-unknown}; shift 2 || true
O=${PROF_OUT:-$R/bench_out}/prof_r5_$TAG
rm -rf "$O"; mkdir -p "$O"
B="python3 $R/bench.py --cpu-rows 0 --no-extras $*"
T="timeout -k 10 240"
$T rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace -- $B --steps 5 --warmup 1 > $O/bench_trace.log 2>&1 &&
$T rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE --output-format csv -d $O/mix -- $B --steps 2 --warmup 0 > $O/mix.log 2>&1 &&
$T rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/fetch -- $B --steps 2 --warmup 0 > $O/fetch.log 2>&1 &&
$T rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/write -- $B --steps 2 --warmup 0 > $O/write.log 2>&1 || { echo "a profiling pass failed: see $O/*.log"; exit 1; }
python3 - "$O" "$REV" "$*" <<'PY'
import collections, csv, glob, json, sys
O, rev, args = sys.argv[1:4]
out = {"git_rev": rev, "bench_args": args}
def per_launch(d, match):
    res = {}
    for f in glob.glob(f"{O}/{d}/*/*_counter_collection.csv"):
        rows = [r for r in csv.DictReader(open(f)) if match(r["Kernel_Name"])]
        agg = collections.defaultdict(float)
        disp = len(set(r["Dispatch_Id"] for r in rows))
        for r in rows:
            agg[r["Counter_Name"]] += float(r["Counter_Value"])
        for k, v in agg.items():
            res[k] = v / max(1, disp)
    return res
for d in ("mix", "fetch", "write"):
    out.update(per_launch(d, lambda n: "render_tiles" in n))
    for name in ("split_finalize", "steal_finalize", "prim_prepass"):
        for k, v in per_launch(d, lambda n: name in n).items():
            out[f"{name}.{k}"] = v
stats = [r for f in glob.glob(f"{O}/trace/*/*_kernel_stats.csv") for r in csv.DictReader(open(f))]
out["kernel_stats"] = [r for r in stats if any(s in r["Name"] for s in ("render", "split", "steal", "prim_prepass"))]
kb = lambda k: out.get(k, 0.0)
tr = {"git_rev": rev, "bench_args": args,
      "render_fetch_kb": kb("FETCH_SIZE"), "render_write_kb": kb("WRITE_SIZE"),
      "split_finalize_fetch_kb": kb("split_finalize.FETCH_SIZE"), "split_finalize_write_kb": kb("split_finalize.WRITE_SIZE"),
      "steal_finalize_fetch_kb": kb("steal_finalize.FETCH_SIZE"), "steal_finalize_write_kb": kb("steal_finalize.WRITE_SIZE"),
      "prim_prepass_fetch_kb": kb("prim_prepass.FETCH_SIZE"), "prim_prepass_write_kb": kb("prim_prepass.WRITE_SIZE")}
tr["bytes_per_launch"] = 1024.0 * sum(v for k, v in tr.items() if k.endswith("_kb"))
json.dump(tr, open(f"{O}/traffic.json", "w"), indent=1)
out["_note"] = ("per launch, headline frame, the kernels of the bench arguments given (default: the tolerance row, --exact: the "
                "bit-exact kernel); FETCH_SIZE / WRITE_SIZE in KB as the counters report them (x 1024 = bytes)")
json.dump(out, open(f"{O}/summary.json", "w"), indent=1)
print(json.dumps({k: v for k, v in out.items() if k != "kernel_stats"}, indent=1))
for r in out["kernel_stats"]:
    print(r["Name"][:60], r.get("Calls"), r.get("TotalDurationNs"), r.get("AverageNs"), r.get("StdDev"))
PY
