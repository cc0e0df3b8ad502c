"""Worst measured fraction of each gate per request kind, from the lines tests/test_gpu_request_kinds.py prints:
    python -m pytest tests/test_gpu_request_kinds.py -m gpu -s | python tests/tools/request_kinds_margins.py
writes the tables of profiles/request_kinds.md to stdout."""
import sys
from collections import defaultdict

worst = defaultdict(lambda: defaultdict(lambda: (0.0, "")))
pairs, switches = [], defaultdict(lambda: (0.0, 0.0, ""))
for line in sys.stdin:
    f = [s.strip() for s in line.split("|")]
    if f[0].endswith("request-kinds margin"):
        group = "fuzz" if "/fuzz-" in f[1] else f[1].split("/")[0]
        for item in f[3:]:
            key, val = item.split()
            if val != "-" and float(val) >= worst[(group, f[2])][key][0]:
                worst[(group, f[2])][key] = (float(val), f[1])
    elif f[0].endswith("request-kinds pair"):
        pairs.append((f[1], f[2], f[3]))
    elif f[0].endswith("request-kinds switch"):
        k = (f[3], f[4], f[2])
        if float(f[6]) >= switches[k][1]:
            switches[k] = (float(f[5]), float(f[6]), f[1])
print("| engine / cases | kind | energy | force | stress | charge |\n|---|---|---|---|---|---|")
for (group, kind), w in sorted(worst.items()):
    print(f"| {group} | {kind} | " + " | ".join(f"{w[k][0]:.3f} ({w[k][1]})" if k in w else "-" for k in ("energy", "force", "stress", "charge")) + " |")
print("\n| pair not bitwise by design | case | max abs difference |\n|---|---|---|")
for case, what, d in pairs:
    print(f"| {what} | {case} | {d} |")
print("\n| switch = 0 | quantity | kind | worst abs difference | fraction of the bound | case |\n|---|---|---|---|---|---|")
for (opt, key, kind), (d, fr, case) in sorted(switches.items()):
    print(f"| {opt} | {key} | {kind} | {d:.3e} | {fr:.3f} | {case} |")
