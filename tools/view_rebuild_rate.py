"""Rebuilds of the active view in a rocprofv3 kernel trace (profiles/view_rebuild/README.md):
every launch of the gather kernels with the frames it moved (its grid: one workgroup of
256 per tile of the view), its time and the rate that makes of `bytes_per_frame` bytes,
and the launch counts and total times of the view's other kernels.

    python3 tools/view_rebuild_rate.py <kernel_trace.csv> <atoms> <out.txt> [moves]

`moves`: how many times ek_view_build_kernel moves a frame's 12 * atoms bytes -- 2 in this
tree (the row read, the quad copy written), 3 for a trace of a tree whose build also wrote a
frame-major copy of the view (profiles/view_rebuild/).
"""
import collections
import csv
import sys

path, atoms, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
moves = int(sys.argv[4]) if len(sys.argv) > 4 else 2
rows = list(csv.DictReader(open(path)))
gx = "Grid_Size_X" if rows and "Grid_Size_X" in rows[0] else "Grid_Size"
# bytes a frame of the view costs: one read of its row and the quad copy
# (ek_view_build_kernel<.., true>), or -- the earlier gather -- the read, a frame-major
# copy and the frame-minor tile
per_frame = {"ek_view_build_kernel": moves * 12 * atoms, "ek_view_gather_kernel": 3 * 12 * atoms}
tot = collections.defaultdict(lambda: [0, 0.0])
lines = []
for r in rows:
    name = r["Kernel_Name"].replace("void ", "").split("(")[0]
    us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    if "ek_view" in name or "ek_quad_tiles" in name:
        tot[name][0] += 1
        tot[name][1] += us
    for k, b in per_frame.items():
        if name.startswith(k):
            # (ek_view_build_kernel: four workgroups of 256 per tile of 256 frames)
            frames = int(r[gx]) // (4 if k == "ek_view_build_kernel" else 1)
            lines.append("%s frames<=%d us=%.1f GB/s=%.0f" % (name, frames, us,
                                                             b * frames / us / 1e3))
with open(out, "w") as fh:
    for name, (n, us) in sorted(tot.items()):
        fh.write("%s launches=%d total_us=%.1f\n" % (name, n, us))
    fh.write("\n".join(lines) + "\n")
print(open(out).read())
