#!/bin/bash
# Profiles the surface renderings on the GPU box: per-kernel timing of tools/time_mesh_render.py (--kernel-trace --stats) and, in SEPARATE
# runs, PMC counters of the raster kernel (issue / wait cycles; LDS; FETCH_SIZE).
#   tools/profile_mesh_render.sh [output directory]      (default: $TMPDIR/prof_mesh)
set -u
OUT=${1:-${TMPDIR:-/tmp}/prof_mesh}
mkdir -p "$OUT"
CMD="python $PWD/tools/time_mesh_render.py"
echo "== kernel trace"
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace" -o trace -- $CMD > "$OUT/trace.log" 2>&1 || { echo "trace failed"; tail -5 "$OUT/trace.log"; exit 1; }
for grp in "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY" \
           "SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VMEM_RD SQ_INSTS_SALU SQ_WAIT_INST_LDS GRBM_GUI_ACTIVE" \
           "FETCH_SIZE"; do
  name=$(echo $grp | cut -d' ' -f1)
  echo "== pmc $grp"
  timeout -k 10 240 rocprofv3 --kernel-trace --pmc $grp --output-format csv -d "$OUT/pmc_$name" -o pmc -- $CMD > "$OUT/pmc_$name.log" 2>&1 || { echo "pmc $name failed"; tail -5 "$OUT/pmc_$name.log"; exit 1; }
done
python - "$OUT" <<'PY'
import collections, csv, glob, os, sys
out = sys.argv[1]
st = glob.glob(os.path.join(out, "trace/**/*kernel_stats.csv"), recursive=True)
with open(os.path.join(out, "mesh_render_kernel_stats.txt"), "w") as f:
    f.write("rocprofv3 --kernel-trace --stats -- python tools/time_mesh_render.py\n")
    f.write(f"{'kernel':<70} {'calls':>6} {'total_ns':>12} {'avg_ns':>10} {'pct':>7}\n")
    for r in list(csv.DictReader(open(st[0])))[:30]:
        f.write(f"{r['Name'][:70]:<70} {r['Calls']:>6} {r['TotalDurationNs']:>12} {float(r['AverageNs']):>10.0f} {r['Percentage']:>7}\n")
with open(os.path.join(out, "mesh_render_pmc.txt"), "w") as f:
    f.write("separate rocprofv3 --kernel-trace --pmc passes of tools/time_mesh_render.py; mean per dispatch by (kernel, workgroups)\n")
    for d in sorted(glob.glob(os.path.join(out, "pmc_*"))):
        c = glob.glob(os.path.join(d, "**/*counter_collection.csv"), recursive=True)
        if not os.path.isdir(d) or not c:
            continue
        agg = collections.defaultdict(lambda: collections.defaultdict(lambda: [0.0, 0]))
        for r in csv.DictReader(open(c[0])):
            k = r.get('Kernel_Name', '?')
            if 'mr_' not in k and 'vn_' not in k and 'depth_mesh' not in k:
                continue
            a = agg[(k[:60], r.get('Grid_Size', '?'))][r['Counter_Name']]
            a[0] += float(r['Counter_Value']); a[1] += 1
        for (k, g), cs in sorted(agg.items()):
            f.write(f"{k}  grid {g}\n")
            for cn, (tot, n) in sorted(cs.items()):
                f.write(f"    {cn:<28} {tot / max(n, 1):.6g}   (n={n})\n")
print(open(os.path.join(out, "mesh_render_kernel_stats.txt")).read())
print(open(os.path.join(out, "mesh_render_pmc.txt")).read())
PY
find "$OUT" -type f -size +2M -delete
