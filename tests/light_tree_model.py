"""The numpy restatement of the light tree: the build over the point and spot lights (object median of the positions, breadth-first
layout), the light table's one entry for them, the walk by power / distance^2 with the number the selection left, and the sample at the leaf, in
float32 with the operand orders the section gives. The records, their selection weights and the sample of a record come from
tests/soft_light_model.py and tests/punctual_model.py. It shares no text with the library: tests/test_light_tree.py holds the host hook to it bit
for bit, tests/test_gpu_light_tree.py the device probe."""
import numpy as np

from tests import punctual_model as pm
from tests import soft_light_model as sm

F = np.float32
TREE_INST = 0xFFFFFFFD
LEAF = 0x80000000
NO_RECORD = 0xFFFFFFFF
MAX_STEPS = 32
P_MIN, P_MAX = F(2.0 ** -16), F(F(1) - F(2.0 ** -16))
U_TOP = F(1 - 2.0 ** -24)  # the largest float32 below 1


def is_local(rec):
    return rec["kind"] != pm.SUN


def tree_exists(mode, records):
    return bool(mode) and sum(1 for r in records if is_local(r)) >= 2


def tree_power(records, weights):
    """the tree's selection weight: the local lights' float32 weights summed in double, in the order given, rounded once"""
    s = 0.0
    for r, w in zip(records, weights):
        if is_local(r):
            s += float(F(w))
    return F(s)


def build(records, weights):
    """records: every punctual light's record in the order given; weights: their float32 selection weights -> the node words, uint32 (2 L - 1, 8):
    lo.xyz, power | hi.xyz, child. (0, 8) with fewer than two local lights."""
    local = [k for k, r in enumerate(records) if is_local(r)]
    if len(local) < 2:
        return np.zeros((0, 8), np.uint32)
    q = {k: np.asarray(records[k]["q"], F) for k in local}
    ranges, child = [local], []
    head = 0
    while head < len(ranges):  # the queue: a range taken off it gives its two halves the next two indices
        items = ranges[head]
        head += 1
        if len(items) == 1:
            child.append(LEAF | items[0])
            continue
        pos = np.stack([q[k] for k in items])
        ext = (pos.max(axis=0) - pos.min(axis=0)).astype(F)
        axis = 0
        for a in (1, 2):
            if ext[a] > ext[axis]:
                axis = a
        ordered = sorted(items, key=lambda k: (float(q[k][axis]), k))
        nl = (len(ordered) + 1) // 2
        child.append(len(ranges))
        ranges.append(ordered[:nl])
        ranges.append(ordered[nl:])
    n = len(ranges)
    lo, hi, power = np.zeros((n, 3), F), np.zeros((n, 3), F), np.zeros(n, F)
    for k in range(n - 1, -1, -1):  # children sit behind their parent
        if child[k] & LEAF:
            r = records[child[k] & ~LEAF]
            rad = F(r.get("radius", 0.0))
            lo[k], hi[k], power[k] = r["q"] - rad, r["q"] + rad, F(weights[child[k] & ~LEAF])
        else:
            a, b = child[k], child[k] + 1
            lo[k], hi[k] = np.minimum(lo[a], lo[b]), np.maximum(hi[a], hi[b])
            power[k] = F(power[a] + power[b])
    words = np.zeros((n, 8), np.uint32)
    words[:, 0:3], words[:, 3], words[:, 4:7] = lo.view(np.uint32), power.view(np.uint32), hi.view(np.uint32)
    words[:, 7] = np.asarray(child, np.uint64).astype(np.uint32)
    return words


def _max_f(a, b):
    return np.where(a > b, a, b).astype(F)


def _min_f(a, b):
    return np.where(a < b, a, b).astype(F)


def _div_s(a, s):
    """a * (1 / s): a division and a multiplication, each rounded"""
    with np.errstate(all="ignore"):
        return (a * (F(1) / s).astype(F)).astype(F)


def importance(words, node, p):
    """float32 importance of the nodes `node` (rows,) at the points p (rows, 3)"""
    lo, hi, power = words[node, 0:3].view(F), words[node, 4:7].view(F), words[node, 3].view(F)
    with np.errstate(all="ignore"):
        c = ((lo + hi) * F(0.5)).astype(F)
        h = ((hi - lo) * F(0.5)).astype(F)
        r2 = pm._dot(h, h)
        d = (p - c).astype(F)
        d2 = pm._dot(d, d)
        return _div_s(power, _max_f(d2, r2))


def left_probability(words, left, p):
    """the clamped probability of the left child `left` (rows,) against its sibling left + 1, at p"""
    with np.errstate(all="ignore"):
        wl, wr = importance(words, left, p), importance(words, left + 1, p)
        s = (wl + wr).astype(F)
        pl = _div_s(wl, s)
        pa, pb = words[left, 3].view(F), words[left + 1, 3].view(F)
        pl = np.where((s > 0) & np.isfinite(s), pl, _div_s(pa, (pa + pb).astype(F))).astype(F)
        return _min_f(_max_f(pl, P_MIN), P_MAX)


def walk(words, p, u, pdf):
    """From the root with the numbers u (rows,), the pdfs coming in (rows,), at the points p (rows, 3) -> pdf, record, reached a leaf, depth, and
    the path: per level the left child's probability (NaN below a row's leaf) and whether the row went left."""
    p, u, pdf = np.ascontiguousarray(p, F), np.asarray(u, F).copy(), np.asarray(pdf, F).copy()
    n = p.shape[0]
    child = np.full(n, words[0, 7], np.uint32)
    depth = np.zeros(n, np.int64)
    levels_pl, levels_left = [], []
    for _ in range(MAX_STEPS):
        act = np.nonzero((child & LEAF) == 0)[0]
        if act.size == 0:
            break
        a = child[act].astype(np.int64)
        pl = left_probability(words, a, p[act])
        ua = u[act]
        left = ua < pl
        with np.errstate(all="ignore"):
            qr = (F(1) - pl).astype(F)
            pdf[act] = np.where(left, pdf[act] * pl, pdf[act] * qr).astype(F)
            un = np.where(left, _div_s(ua, pl), _div_s((ua - pl).astype(F), qr)).astype(F)
        u[act] = _min_f(un, U_TOP)
        child[act] = np.where(left, words[a, 7], words[a + 1, 7])
        depth[act] += 1
        lp, ll = np.full(n, np.nan, F), np.zeros(n, bool)
        lp[act], ll[act] = pl, left
        levels_pl.append(lp)
        levels_left.append(ll)
    ok = (child & LEAF) != 0
    return pdf, (child & ~np.uint32(LEAF)).astype(np.uint32), ok, depth, (levels_pl, levels_left)


def record_pdfs(words, records, p):
    """the probability the walk gives every record at the points p (rows, 3), whatever u: (rows, len(records)) float32 (0 for a sun), the products
    taken from the root down as the walk takes them; and every record's depth"""
    p = np.ascontiguousarray(p, F)
    n, rows = words.shape[0], p.shape[0]
    prob = np.zeros((n, rows), F)
    prob[0] = 1
    level = np.zeros(n, np.int64)
    out, depth = np.zeros((rows, len(records)), F), np.zeros(len(records), np.int64)
    for k in range(n):
        c = int(words[k, 7])
        if c & LEAF:
            out[:, c & ~LEAF], depth[c & ~LEAF] = prob[k], level[k]
            continue
        pl = left_probability(words, np.full(rows, c, np.int64), p)
        prob[c], prob[c + 1] = prob[k] * pl, prob[k] * (F(1) - pl).astype(F)
        level[c] = level[c + 1] = level[k] + 1
    return out, depth


def alias_pick_remap(j, t, pdf, u):
    """punctual_model.alias_pick with the number the step leaves for the next: (index, its pdf, u remapped)"""
    n = len(j)
    u = np.asarray(u, F)
    fn = F(n)
    i = np.clip(np.floor(u * fn).astype(np.int64), 0, n - 1)
    with np.errstate(all="ignore"):
        u1 = (u * fn - i.astype(F)).astype(F)
        first = u1 < t[i]
        u2 = np.where(first, u1 / t[i], (u1 - t[i]).astype(F) / (F(1) - t[i]).astype(F)).astype(F)
    idx = np.where(first, i, j[i].astype(np.int64))
    return idx, pdf[idx], u2


def table_entries(mode, n_mesh_lights, records, env):
    """the light table's entries in order, with a tree or without: ("mesh", k), ("punct", record), ("tree", None), ("env", None)"""
    tree = tree_exists(mode, records)
    out = [("mesh", k) for k in range(n_mesh_lights)]
    out += [("punct", k) for k, r in enumerate(records) if not tree or not is_local(r)]
    if tree:
        out.append(("tree", None))
    if env:
        out.append(("env", None))
    return out


def light_sample_rows(table, entries, records, words, rows):
    """table: (j, t, pdf) of the light list; entries: table_entries' list; records: every punctual record in the order given; words: build's nodes;
    rows (n, 9) = p, n, u_select, u_sample -> (out (n, 13), light (n,), record (n,)) as akr_host_light_tree_sample answers, and the walk's path"""
    rows = np.ascontiguousarray(rows, F).reshape(-1, 9)
    n = rows.shape[0]
    idx, pdf, u2 = alias_pick_remap(table[0], table[1], table[2], rows[:, 6])
    out = np.zeros((n, 13), F)
    out[:, 6] = pdf
    record = np.full(n, NO_RECORD, np.uint32)
    which = np.full(n, -1, np.int64)  # the record to sample
    path = None
    for l, (kind, k) in enumerate(entries):
        sel = np.nonzero(idx == l)[0]
        if sel.size == 0:
            continue
        if kind == "punct":
            which[sel] = k
        elif kind == "tree":
            tp, trec, ok, _, path_sel = walk(words, rows[sel, 0:3], u2[sel], pdf[sel])
            out[sel, 6], out[sel, 12] = tp, 1.0
            record[sel] = trec
            which[sel[ok]] = trec[ok]
            path = (sel, path_sel)
    for k, rec in enumerate(records):
        sel = np.nonzero(which == k)[0]
        if sel.size == 0:
            continue
        li, wi, ro, tmax, valid = sm.sample(rec, rows[sel, 0:3], rows[sel, 3:6], rows[sel, 7:9])
        o = out[sel]
        o[:, 0:3], o[:, 3:6], o[:, 7:10], o[:, 10], o[:, 11], o[:, 12] = li, wi, ro, tmax, valid.astype(F), 1.0
        out[sel] = o
    return (out, idx.astype(np.uint32), record), path


def thresholds(path_levels, u0):
    """For ONE row that went through a table whose only entry is the tree (u_sel2 = u_select): the u_select values, in float64, at which each level of
    its path branches -- the interval of u_select that reaches a level is [a, b), its threshold a + pl (b - a)."""
    levels_pl, levels_left = path_levels
    a, b, out = 0.0, 1.0, []
    for pl, left in zip(levels_pl, levels_left):
        if np.isnan(pl):
            break
        t = a + float(pl) * (b - a)
        out.append(t)
        a, b = (a, t) if left else (t, b)
    return out
