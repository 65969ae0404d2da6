"""frame_compose_kernel's own times out of a ``rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_render.py
--compose-only`` run: ``python tools/render_kernel_times.py DIR`` prints min / median / max per run of launches with the same grid and
a similar duration (bench_render.py launches every (size, panel set) 22 times in a row; 21 panels are two launches, 16 + 5)."""
import csv, glob, sys
f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
rows = [r for r in csv.DictReader(open(f)) if r["Kernel_Name"].startswith("frame_compose_kernel")]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
groups = []
for r in rows:
    g, d = int(r["Grid_Size_X"]) // 256, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    if groups and groups[-1][0] == g and abs(d - groups[-1][1][0]) < 0.5 * groups[-1][1][0]:
        groups[-1][1].append(d)
    else:
        groups.append((g, [d]))
merged = {}
for g, v in groups:
    key = (g, round(sorted(v)[len(v) // 2], -3 if v[0] > 20000 else -2))
    merged.setdefault(key, []).extend(v)
for (g, _), v in merged.items():
    v.sort()
    print(f"blocks {g:5d}  calls {len(v):3d}  min {v[0] / 1e3:8.2f} us  median {v[len(v) // 2] / 1e3:8.2f} us  max {v[-1] / 1e3:8.2f} us")
print("VGPR", rows[0]["VGPR_Count"], "LDS", rows[0]["LDS_Block_Size"], "scratch", rows[0]["Scratch_Size"])
