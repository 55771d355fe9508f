"""usage: launch_list_diff.py A.json B.json -- the launches (tools/launch_list.py) that differ between two steps, with their durations."""
import json, sys
from collections import Counter
a, b = (json.load(open(p)) for p in sys.argv[1:3])
key = lambda r: (r[0], tuple(r[1]), tuple(r[2]))
ca, cb = Counter(key(r) for r in a["launches"]), Counter(key(r) for r in b["launches"])
print(f"{sys.argv[1]}: {a['n']} launches   {sys.argv[2]}: {b['n']} launches")
print("same multiset of (kernel, grid, block):", ca == cb, "  same order:", [key(r) for r in a["launches"]] == [key(r) for r in b["launches"]])
for k in sorted(set(ca) | set(cb)):
    if ca[k] != cb[k]:
        ua = [r[3] for r in a["launches"] if key(r) == k]; ub = [r[3] for r in b["launches"] if key(r) == k]
        print(f"  {ca[k]} -> {cb[k]}  {k[0][:100]} grid {k[1]}  us {['%.1f' % u for u in ua]} -> {['%.1f' % u for u in ub]}")
