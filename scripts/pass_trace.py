"""Linearisation launches of a rocprofv3 --kernel-trace CSV (scripts/run_probe.py under the profiler), by structure: the advance pass
with the linearisation kernel behind it (k_advance, gap, k_lin), the pass alone (k_advance ROWS) and the linearisation kernel alone.
usage: pass_trace.py <..._kernel_trace.csv> [launches of the LAST n linearisations, default 100]"""
import csv, sys
import numpy as np

rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        name = r["Kernel_Name"]
        short = "k_advance_team" if "k_advance_team" in name else "k_advance" if "k_advance" in name else "k_lin" if "k_lin<" in name else \
                "k_sum_tiles" if "k_sum_tiles" in name else "k_gate" if "k_gate" in name else None
        if short:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short))
rows.sort()
last = int(sys.argv[2]) if len(sys.argv) > 2 else 100
# a launch: [k_gate] [k_advance] [k_lin [k_sum_tiles]]
launches, cur = [], []
for s, e, k in rows:
    if k == "k_gate" or (cur and cur[-1][2] not in ("k_gate",) and k in ("k_advance", "k_advance_team")) or (cur and cur[-1][2] in ("k_lin", "k_sum_tiles") and k == "k_lin") \
            or (cur and cur[-1][2] == "k_advance" and k == "k_advance"):
        if cur:
            launches.append(cur)
        cur = []
    cur.append((s, e, k))
if cur:
    launches.append(cur)
launches = launches[-last:]
us = lambda ns: ns / 1e3
two, alone, plain = [], [], []
print("launch  structure                 kernels (us)                          first start -> last end (us)")
for i, L in enumerate(launches):
    ks = [x for x in L if x[2] != "k_gate"]
    names = [x[2] for x in ks]
    span = us(ks[-1][1] - ks[0][0])
    parts = " ".join("%s %.1f" % (k, us(e - s)) for s, e, k in ks)
    if names[:2] == ["k_advance", "k_lin"]:
        gap = us(ks[1][0] - ks[0][1])
        two.append((us(ks[0][1] - ks[0][0]), gap, us(ks[1][1] - ks[1][0]), span))
        parts += " gap %.1f" % gap
        st = "pass + k_lin"
    elif names == ["k_advance"]:
        alone.append(span); st = "pass alone"
    else:
        plain.append(span); st = "+".join(names)
    print("%4d    %-24s  %-44s %.1f" % (i, st, parts, span))
if two:
    a = np.array(two)
    print("pass + k_lin: %d launches; k_advance %.1f, gap %.1f, k_lin %.1f, span %.1f us (means); span sum %.0f us" % ((len(a),) + tuple(a.mean(0)) + (a[:, 3].sum(),)))
if alone:
    print("pass alone  : %d launches; %.1f us (mean); sum %.0f us" % (len(alone), np.mean(alone), np.sum(alone)))
if plain:
    print("k_lin alone : %d launches; %.1f us (mean); sum %.0f us" % (len(plain), np.mean(plain), np.sum(plain)))
