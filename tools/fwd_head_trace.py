"""The head of the rasterizer forward in a rocprofv3 kernel trace: python tools/fwd_head_trace.py <dir or csv> [skip].

For every forward (one preprocess_kernel dispatch) after the first `skip` (default 10, the warm-up): the
interval from the end of preprocess_kernel to the start of emit_instances_kernel and to the start of
render_forward_kernel, and the durations of the kernels between them.  Prints medians, minima and maxima in us."""
import csv
import glob
import os
import statistics
import sys

HEAD = ("visible_scan_kernel", "emit_instances_kernel", "tile_count_kernel", "tile_scan_kernel",
        "tile_scatter_kernel", "tile_sort_kernel", "render_forward_kernel")


def rows(path):
    if os.path.isdir(path):
        found = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
        if not found:
            sys.exit(f"no *kernel_trace.csv under {path}")
        path = found[0]
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            yield r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])


def short(name):
    for k in ("preprocess_kernel",) + HEAD:
        if k in name and "backward" not in name:
            return k
    return None


def main():
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    ev = sorted((s, e, short(n)) for n, s, e in rows(sys.argv[1]) if short(n))
    fwds, cur = [], None
    for s, e, k in ev:
        if k == "preprocess_kernel":
            cur = {"pre_end": e}
            fwds.append(cur)
        elif cur is not None and k not in cur:   # the first dispatch of each kernel after the preprocess
            cur[k] = (s, e)
    fwds = [f for f in fwds[skip:] if "emit_instances_kernel" in f and "render_forward_kernel" in f]
    if not fwds:
        sys.exit("no complete forward in the trace")

    def stat(name, vals):
        vals = [v / 1e3 for v in vals]
        print(f"{name:42s} median {statistics.median(vals):7.2f}  min {min(vals):7.2f}  max {max(vals):7.2f} us")

    print(f"{len(fwds)} forwards (first {skip} skipped)")
    stat("preprocess end -> emit_instances start", [f["emit_instances_kernel"][0] - f["pre_end"] for f in fwds])
    stat("preprocess end -> render_forward start", [f["render_forward_kernel"][0] - f["pre_end"] for f in fwds])
    for k in HEAD[:-1]:
        d = [f[k][1] - f[k][0] for f in fwds if k in f]
        if d:
            stat(k + " duration", d)


if __name__ == "__main__":
    main()
