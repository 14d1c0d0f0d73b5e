"""Numpy / plain-Python restatement of the connectivity-by-module rules
(include/netrep_gpu.h has them): the module-connectivity table in its stated
summation order, the intramodular connectivity, the eigengene tree with
average and complete linkage and its tie rule, and the node and sample
orders built from them."""
import math

import numpy as np

import hclust_ref as H
import modmerge_ref as R


def slots_of(labels):
    """slot[j]: the index of node j's label among the distinct positive
    labels in increasing order, -1 for label 0; and those labels."""
    labels = np.asarray(labels)
    mods = R.modules_of(labels)
    slot = np.full(labels.size, -1, dtype=np.int32)
    sel = labels > 0
    slot[sel] = np.searchsorted(mods, labels[sel]).astype(np.int32)
    return slot, mods


def ordered_sum(w):
    """The contract's sum of every column of w (rows x columns, >= 0, the
    rows that do not take part zeroed: adding +0.0 changes no bit of a
    non-negative partial): 64 partials, partial l adding rows l, l + 64, ...
    in increasing order from +0.0, then p[l] += p[l + off], off = 32 .. 1."""
    rows, cols = w.shape
    p = np.zeros((64, cols))
    for r0 in range(0, rows, 64):
        blk = w[r0:r0 + 64]
        p[:blk.shape[0]] += blk
    off = 32
    while off:
        p[:off] += p[off:2 * off]
        off //= 2
    return p[0].copy()


def module_connectivity(net, slot, n_mod):
    """(k_mod [n x n_mod], k_total [n]) of net (n x n; element (j, i) is row
    j of column i) in the stated order."""
    a = np.abs(np.asarray(net, dtype=np.float64)).copy()
    np.fill_diagonal(a, 0.0)
    slot = np.asarray(slot)
    k_mod = np.zeros((a.shape[0], n_mod), order="F")
    for m in range(n_mod):
        k_mod[:, m] = ordered_sum(np.where((slot == m)[:, None], a, 0.0))
    return k_mod, ordered_sum(a)


def fsum_table(net, slot, n_mod):
    """The same table with every cell the exactly rounded sum (math.fsum)."""
    a = np.abs(np.asarray(net, dtype=np.float64)).copy()
    np.fill_diagonal(a, 0.0)
    n = a.shape[0]
    k_mod = np.zeros((n, n_mod), order="F")
    for m in range(n_mod):
        rows = a[np.asarray(slot) == m]
        k_mod[:, m] = [math.fsum(rows[:, i].tolist()) for i in range(n)]
    return k_mod, np.array([math.fsum(a[:, i].tolist()) for i in range(n)])


def intramodular(slot, k_total, k_mod):
    """kWithin, kOut, kDiff; NaN all three for slot -1."""
    slot = np.asarray(slot)
    n = slot.size
    within = np.full(n, np.nan)
    sel = slot >= 0
    within[sel] = np.asarray(k_mod)[np.flatnonzero(sel), slot[sel]]
    out = np.asarray(k_total) - within
    return within, out, within - out


def eigengene_tree(eig, linkage):
    """netrep_EigengeneTree in plain Python floats, operation by operation:
    the globally closest pair of clusters each step, ties to the lowest
    (lower, higher) pair, a cluster indexed by its lowest column; "average"
    (Lance-Williams, never fused) or "complete" (the larger distance).
    Returns (id_lo, id_hi, height) in discovery order and the merged column
    sets per step."""
    d = R.eigengene_dissimilarity(eig)
    m = len(d)
    size = [1.0] * m
    live = [True] * m
    ident = list(range(m))
    members = [{j} for j in range(m)]
    id_lo, id_hi, heights, sets = [], [], [], []
    for step in range(m - 1):
        best = None
        for i in range(m):
            if not live[i]:
                continue
            for j in range(i + 1, m):
                if live[j] and (best is None or d[i][j] < best[0]):
                    best = (d[i][j], i, j)
        h, i, j = best
        heights.append(h)
        id_lo.append(ident[i])
        id_hi.append(ident[j])
        si, sj = size[i], size[j]
        for k in range(m):
            if live[k] and k != i and k != j:
                if linkage == "complete":
                    v = max(d[k][i], d[k][j])
                else:
                    v = (si * d[k][i] + sj * d[k][j]) / (si + sj)
                d[k][i] = d[i][k] = v
        size[i] = si + sj
        live[j] = False
        ident[i] = m + step
        members[i] = members[i] | members[j]
        sets.append(frozenset(members[i]))
    return (np.array(id_lo, dtype=np.int32), np.array(id_hi, dtype=np.int32), np.array(heights, dtype=np.float64),
            sets)


def module_order(eig, mods):
    """The labels in the leaf order of the complete-linkage tree of their
    eigengenes (R's hclust(as.dist(1 - cor(summaries)))$order)."""
    mods = [int(m) for m in mods]
    if len(mods) < 2:
        return mods
    id_lo, id_hi, height, _sets = eigengene_tree(eig, "complete")
    _merge, _h, order, _repairs = H.finish(len(mods), id_lo, id_hi, height)
    return [mods[int(o) - 1] for o in order]


def node_order(labels, k_within, names, mod_order):
    """Per module of mod_order the names by decreasing kWithin, ties keeping
    node order (R's sort(decreasing = TRUE) is stable); flattened too."""
    labels = np.asarray(labels)
    per = {}
    for m in mod_order:
        idx = np.flatnonzero(labels == m).tolist()
        idx.sort(key=lambda i: -k_within[i])                    # list.sort is stable
        per[int(m)] = [names[i] for i in idx]
    return [nm for m in mod_order for nm in per[int(m)]], per


def sample_order(eig, mods):
    """Per module the 0-based sample indices by decreasing eigengene value,
    ties in sample order (R's order(decreasing = TRUE))."""
    out = {}
    for j, m in enumerate(mods):
        col = np.asarray(eig)[:, j].tolist()
        out[int(m)] = np.array(sorted(range(len(col)), key=lambda s: -col[s]), dtype=np.int64)
    return out
