"""Numpy restatement of what follows a cut (include/netrep_gpu.h has the
rules): module eigengenes, module membership, the eigengene tree and its cut,
the merging and relabelling of labels, the mergeCloseModules loop and the kME
trimming -- and the generator of data with planted, partly correlated
modules that the tests of both run on."""
import math

import numpy as np


def scale(x):
    """Scale (src/scale.cpp): per-column (x - mean) / sd, sd with n - 1."""
    x = np.asarray(x, dtype=np.float64)
    return np.asfortranarray((x - x.mean(axis=0)) / x.std(axis=0, ddof=1))


def modules_of(labels):
    labels = np.asarray(labels)
    return np.unique(labels[labels > 0]).astype(np.int32)


def eigengene(cols):
    """NetRep's summary profile of the columns (src/netStats.cpp:217-250):
    the first left singular vector, its sign such that it correlates
    positively with the mean of the columns. Returns it and the singular
    values."""
    u, sv, _vt = np.linalg.svd(cols, full_matrices=False)
    e = u[:, 0]
    if np.corrcoef(cols.mean(axis=1), e)[0, 1] < 0:
        e = -e
    return e, sv


def cor_columns(x, e):
    """Pearson correlation of every column of x with every column of e, by
    centred dot products."""
    xc = x - x.mean(axis=0)
    ec = e - e.mean(axis=0)
    return (xc.T @ ec) / np.sqrt((xc * xc).sum(axis=0))[:, None] / np.sqrt((ec * ec).sum(axis=0))[None, :]


def module_eigengenes(data, labels):
    """Of the data as given (scale first for a scaled handle): modules,
    eigengenes (S x M), varExplained (the mean squared own kME), own kME (n,
    NaN for label 0) and the smallest relative gap between a module's top two
    singular values."""
    labels = np.asarray(labels)
    mods = modules_of(labels)
    s = data.shape[0]
    eig = np.zeros((s, mods.size), order="F")
    ve = np.zeros(mods.size)
    own = np.full(labels.size, np.nan)
    gap = np.inf
    for j, m in enumerate(mods):
        sel = np.flatnonzero(labels == m)
        eig[:, j], sv = eigengene(data[:, sel])
        if sv.size > 1:
            gap = min(gap, (sv[0] - sv[1]) / sv[0])
        own[sel] = cor_columns(data[:, sel], eig[:, j:j + 1])[:, 0]
        ve[j] = np.mean(own[sel] ** 2)
    return {"modules": mods, "eigengenes": eig, "varExplained": ve, "kME": own, "gap": gap}


def eigengene_dissimilarity(eig):
    """d = 1 - cor(E) as netrep_EigengeneGroups defines it, in plain Python
    floats, operation by operation (a list of rows)."""
    eig = np.asarray(eig, dtype=np.float64)
    s, m = eig.shape
    z, ss = [], []
    for a in range(m):
        total = 0.0
        for v in eig[:, a].tolist():
            total += v
        mean = total / s
        col = [v - mean for v in eig[:, a].tolist()]
        q = 0.0
        for v in col:
            q += v * v
        z.append(col)
        ss.append(q)
    d = [[0.0] * m for _ in range(m)]
    for a in range(m):
        for b in range(a + 1, m):
            dot = 0.0
            for u, v in zip(z[a], z[b]):
                dot += u * v
            c = dot / math.sqrt(ss[a] * ss[b])
            c = min(1.0, max(-1.0, c))
            d[a][b] = d[b][a] = 1.0 - c
    return d


def eigengene_groups(eig, cut_height):
    """netrep_EigengeneGroups in plain Python floats, operation by operation
    (so the heights carry the library's bits): (group, heights)."""
    d = eigengene_dissimilarity(eig)
    m = len(d)
    size = [1.0] * m
    live = [True] * m
    group = list(range(m))
    heights = []
    for _step in range(m - 1):
        best = None
        for i in range(m):
            if not live[i]:
                continue
            for j in range(i + 1, m):
                if live[j] and (best is None or d[i][j] < best[0]):
                    best = (d[i][j], i, j)
        h, i, j = best
        heights.append(h)
        si, sj = size[i], size[j]
        for k in range(m):
            if live[k] and k != i and k != j:
                d[k][i] = d[i][k] = (si * d[k][i] + sj * d[k][j]) / (si + sj)
        size[i] = si + sj
        live[j] = False
        if h <= cut_height:
            group = [i if g == j else g for g in group]
    return np.array(group, dtype=np.int32), np.array(heights, dtype=np.float64)


def relabel_by_size(labels):
    """Positive labels renumbered 1, 2, ... by decreasing size, ties to the
    lower old label. Returns the labels and the old label of each new one."""
    labels = np.asarray(labels, dtype=np.int32)
    mods = modules_of(labels)
    counts = [int((labels == m).sum()) for m in mods]
    order = sorted(range(mods.size), key=lambda j: (-counts[j], int(mods[j])))
    out = labels.copy()
    for new, j in enumerate(order):
        out[labels == mods[j]] = new + 1
    return out, [int(mods[j]) for j in order]


def merge_labels(labels, module_labels, group, relabel=False):
    labels = np.asarray(labels, dtype=np.int32)
    out = labels.copy()
    for m, g in zip(module_labels, group):
        out[labels == m] = module_labels[g]
    return relabel_by_size(out)[0] if relabel else out


def merge_close_modules(data, labels, cut_height, relabel=True):
    """The mergeCloseModules loop on the data as given. Returns labels,
    rounds (those that merged something), the last round's eigengenes (columns
    in the returned labels' module order) and heights, and the heights of
    every round (for the margin precondition)."""
    labels = np.asarray(labels, dtype=np.int32).copy()
    rounds, all_heights = 0, []
    while True:
        r = module_eigengenes(data, labels)
        mods, eig = r["modules"], r["eigengenes"]
        heights = np.zeros(0)
        if mods.size == 1:
            break
        group, heights = eigengene_groups(eig, cut_height)
        all_heights.append(heights)
        if (group == np.arange(mods.size)).all():
            break
        labels = merge_labels(labels, mods, group)
        rounds += 1
    if relabel:
        labels, old = relabel_by_size(labels)
        eig = np.asfortranarray(eig[:, [int(np.searchsorted(mods, o)) for o in old]])
    return {"labels": labels, "rounds": rounds, "eigengenes": eig, "heights": heights, "all_heights": all_heights}


def margin(all_heights, cut_height):
    """Smallest distance of any height of any round from the cut."""
    return min((float(np.abs(h - cut_height).min()) for h in all_heights if h.size), default=np.inf)


def trim_modules(labels, kme_own, min_size, min_kme_to_stay=0.3, min_core_kme=0.5, min_core_kme_size=None):
    labels = np.asarray(labels, dtype=np.int32)
    kme_own = np.asarray(kme_own, dtype=np.float64)
    core_size = -(-min_size // 3) if min_core_kme_size is None else min_core_kme_size
    out = labels.copy()
    for m in modules_of(labels):
        sel = labels == m
        if int((kme_own[sel] > min_core_kme).sum()) < core_size:
            out[sel] = 0
            continue
        drop = sel & (kme_own < min_kme_to_stay)
        out[drop] = 0
        if int(sel.sum() - drop.sum()) < min_size:
            out[sel] = 0
    return out


# The seven-module example: modules 1-2 share a factor at 0.95, 3-4-5 form a
# chain at 0.88 / 0.70, 6 and 7 stand alone. links[m] = (parent, rho): module
# m's factor is rho x the parent's + sqrt(1 - rho^2) x its own.
SEVEN_LINKS = {2: (1, 0.95), 4: (3, 0.88), 5: (4, 0.70)}
SEVEN_GROUPING = [{1, 2}, {3, 4, 5}, {6}, {7}]


def planted(n, s, sizes, links, seed, noise=0.5, negative=0.15, n_noise_inside=0):
    """Data (s x n, raw) with planted modules: module m (label m, sizes[m - 1]
    contiguous nodes, decreasing sizes keep cutreeStatic's numbering) is
    driven by its latent factor, a fraction `negative` of its genes loading
    negatively; the nodes left over are noise with label 0. n_noise_inside:
    that many genes of every module are pure noise (for the trimming).
    Returns the data and the labels."""
    rng = np.random.default_rng([seed, 7])
    sizes = list(sizes)
    assert sum(sizes) <= n
    f = {}
    for m in range(1, len(sizes) + 1):
        own = rng.standard_normal(s)
        if m in links:
            parent, rho = links[m]
            own = rho * f[parent] + math.sqrt(1.0 - rho * rho) * own
        f[m] = own
    x = rng.standard_normal((s, n))
    labels = np.zeros(n, dtype=np.int32)
    at = 0
    for m, k in enumerate(sizes, start=1):
        load = rng.uniform(0.7, 1.0, k)
        n_neg = int(negative * k)
        load[k - n_neg:] *= -1.0
        block = f[m][:, None] * load[None, :] + noise * rng.standard_normal((s, k))
        if n_noise_inside:
            block[:, :n_noise_inside] = rng.standard_normal((s, n_noise_inside))
        x[:, at:at + k] = block
        labels[at:at + k] = m
        at += k
    return np.asfortranarray(x), labels


def grouping_of(labels_before, labels_after):
    """The partition of the old modules that the new labels induce."""
    groups = {}
    for m in modules_of(labels_before):
        new = np.unique(np.asarray(labels_after)[np.asarray(labels_before) == m])
        assert new.size == 1
        groups.setdefault(int(new[0]), set()).add(int(m))
    return sorted(groups.values(), key=min)


def find_seed(n, s, sizes, links, cut_height, rounds, grouping=None, min_margin=0.01, start=0, tries=400, **kw):
    """The first seed from `start` whose planted data need exactly `rounds`
    merging rounds at cut_height with every height of every round at least
    min_margin from the cut (and, if given, end in `grouping`)."""
    for seed in range(start, start + tries):
        x, labels = planted(n, s, sizes, links, seed, **kw)
        r = merge_close_modules(scale(x), labels, cut_height, relabel=False)
        if r["rounds"] != rounds or margin(r["all_heights"], cut_height) < min_margin:
            continue
        if grouping is not None and grouping_of(labels, r["labels"]) != sorted(grouping, key=min):
            continue
        return seed
    raise AssertionError("no seed meets the preconditions")
