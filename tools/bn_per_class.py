"""join the per-launch tables of the two trees: combine + apply (base) vs apply with the combine inside (tree), per tile-count class"""
import re, sys, collections
def load(p):
    rows = []
    for l in open(p):
        m = re.match(r"\s*(\d+) (\S+)\s+([\d.]+) us .*? ([\d.]+) MB\s+[\d.]+ GB/s\s+(.*)", l)
        if m: rows.append((m.group(2), float(m.group(3)), float(m.group(4)), m.group(5).strip()))
    return rows
base, tree = load(sys.argv[1]), load(sys.argv[2])
COMB = {"bn_finalize_tiles": "scale_shift_act", "bn_bwd_sum_tiles": "bn_act_bwd_apply"}
# base: (combine, apply) pairs in launch order; tree: the apply launches in the same order
pairs, i = [], 0
while i < len(base):
    n, us, mb, d = base[i]
    if n in COMB and i + 1 < len(base) and base[i + 1][0] == COMB[n]:
        tiles = int(re.match(r"\((\d+),", d).group(1))
        pairs.append((COMB[n], tiles, us, base[i + 1][1], base[i + 1][3])); i += 2
    else:
        i += 1
INV = {v: k for k, v in COMB.items()}
# (a tree launch above the limit still has its combine launch in front: its time counts into "one")
applies = {k: [(r[0], r[1] + (tree[j - 1][1] if j and tree[j - 1][0] == INV[k] else 0.0), r[2], r[3] + (" +combine" if j and tree[j - 1][0] == INV[k] else ""))
               for j, r in enumerate(tree) if r[0] == k] for k in COMB.values()}
bapplies = {k: [j for j, r in enumerate(base) if r[0] == k] for k in COMB.values()}
# index of each paired apply among the base's applies of that name == its index among the tree's
pos = {k: {} for k in COMB.values()}
for k in COMB.values():
    for idx, j in enumerate(bapplies[k]): pos[k][j] = idx
agg = collections.defaultdict(lambda: [0, 0.0, 0.0, 0.0, 0])
i = 0
while i < len(base):
    n = base[i][0]
    if n in COMB and i + 1 < len(base) and base[i + 1][0] == COMB[n]:
        k = COMB[n]; tiles = int(re.match(r"\((\d+),", base[i][3]).group(1))
        t = applies[k][pos[k][i + 1]]
        a = agg[(k, tiles)]
        a[0] += 1; a[1] += base[i][1]; a[2] += base[i + 1][1]; a[3] += t[1]; a[4] += not t[3].endswith("+combine")
        i += 2
    else:
        i += 1
print(f"{'apply':18s} {'tiles':>6s} {'n':>4s} {'combine':>9s} {'apply':>9s} {'two':>9s} {'one':>9s} {'saved/launch':>13s} {'fused':>6s}   (us, mean per launch)")
for (k, tiles), (n, c, a, f, nf) in sorted(agg.items()):
    print(f"{k:18s} {tiles:6d} {n:4d} {c / n:9.2f} {a / n:9.2f} {(c + a) / n:9.2f} {f / n:9.2f} {(c + a - f) / n:13.2f} {nf:6d}")
