#!/usr/bin/env python
"""Mean duration per launch POSITION in the frame from a rocprofv3 --kernel-trace database (rocpd sqlite) of a one-frame-in-flight bench run (the table of
profiles/r*_kernel_trace_by_launch.json): k_shade[b] = shade of bounce b, k_trace_fused[i] = fused launch i + 1, and so on.  A frame
ends with its k_gather; frames whose launch list differs from the most common one (warm-up, the profiled frames of --full) are left out.
usage: tools/kernel_trace_by_launch.py <results.db> [label]    (prints one JSON object)"""
import collections
import json
import sqlite3
import sys


def base(name):
    n = name.split("(")[0].replace("void ", "").replace("atn::", "")
    return n.split("<")[0], name.split("(")[0]


def main():
    rows = list(sqlite3.connect(sys.argv[1]).execute("select start, end, name from kernels order by start"))
    frames, cur = [], []
    for s, e, n in rows:
        b, full = base(n)
        if not b.startswith("k_"):
            continue
        cur.append((b, full, (e - s) / 1e3))
        if b == "k_gather":
            frames.append(cur)
            cur = []
    shape = collections.Counter(tuple(b for b, _, _ in f) for f in frames).most_common(1)[0][0]
    frames = [f for f in frames if tuple(b for b, _, _ in f) == shape]
    out = collections.OrderedDict(frames=len(frames))
    acc, kern = collections.defaultdict(list), {}
    for f in frames:
        pos = collections.Counter()
        for b, full, us in f:
            key = "%s[%d]" % (b, pos[b])
            pos[b] += 1
            acc[key].append(us)
            kern[key] = full
    per = collections.defaultdict(float)
    for key in sorted(acc):
        v = acc[key]
        mean = sum(v) / len(v)
        sd = (sum((x - mean) ** 2 for x in v) / len(v)) ** 0.5
        out[key] = dict(mean_us=round(mean, 2), sd_us=round(sd, 2), n=len(v), kernel=kern[key])
        per[key.split("[")[0]] += mean / 1e3
    out["per_frame_ms"] = {k: round(v, 4) for k, v in per.items()}
    print(json.dumps({sys.argv[2] if len(sys.argv) > 2 else "run": out}, indent=1))


if __name__ == "__main__":
    main()
