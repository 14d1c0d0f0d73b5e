"""numpy restatement of the average-linkage dendrogram and the static cut
(include/netrep_gpu.h, nr_hclust_average / netrep_HclustFinish /
netrep_CutreeStatic), as the test oracle.

The chain: nearest-neighbour chain on d = 1 - net (+inf on the diagonal) with
fixed rules, so that the output is a function of the input alone:
  * the merged cluster lives in slot hi = max(a, b); slot lo is retired (its
    row and column become +inf);
  * an empty chain starts at the lowest-index live slot;
  * the nearest neighbour of the chain's top a is the live k != a with the
    smallest d(a, k), the lowest index on ties -- except that the chain's
    previous element is chosen whenever it attains the minimum;
  * when the nearest neighbour is the previous element the two are merged at
    height d(a, b), both are popped and the rest of the chain is kept;
  * d(k, a u b) = (s_a d(k, a) + s_b d(k, b)) / (s_a + s_b), every operation
    rounded on its own (numpy ufuncs never fuse);
  * merges are emitted in discovery order as (id_lo, id_hi, height, size): the
    ids of the clusters in slots lo and hi, 0 .. n-1 nodes, n + t the cluster
    of discovery step t.
"""
import numpy as np


def chain(d):
    """(id_lo, id_hi, height, size, searches) of a square dissimilarity (its
    diagonal is ignored)."""
    D = np.array(d, dtype=np.float64)
    n = D.shape[0]
    assert D.shape == (n, n)
    np.fill_diagonal(D, np.inf)
    size = np.ones(n)
    ids = np.arange(n, dtype=np.int64)
    id_lo = np.zeros(max(n - 1, 0), np.int32)
    id_hi = np.zeros(max(n - 1, 0), np.int32)
    height = np.zeros(max(n - 1, 0))
    msize = np.zeros(max(n - 1, 0))
    stack, first, searches, t = [], 0, 0, 0
    while t < n - 1:
        assert searches < search_cap(n), "the chain exceeded its search cap"
        if not stack:
            while size[first] == 0.0:
                first += 1
            stack.append(first)
        a = stack[-1]
        prev = stack[-2] if len(stack) >= 2 else -1
        col = D[:, a]
        k = int(np.argmin(col))               # the first (lowest) index of the minimum
        m = col[k]
        searches += 1
        assert np.isfinite(m), "no finite neighbour"
        if prev >= 0 and col[prev] == m:
            k = prev
        if k != prev:
            stack.append(k)
            continue
        lo, hi = min(a, k), max(a, k)
        sa, sb = size[lo], size[hi]
        tot = sa + sb
        new = (sa * D[:, lo] + sb * D[:, hi]) / tot
        new[lo] = new[hi] = np.inf
        D[:, hi] = new
        D[hi, :] = new
        D[:, lo] = np.inf
        D[lo, :] = np.inf
        id_lo[t], id_hi[t], height[t], msize[t] = ids[lo], ids[hi], m, tot
        ids[hi] = n + t
        size[hi], size[lo] = tot, 0.0
        del stack[-2:]
        t += 1
    return id_lo, id_hi, height, msize, searches


def search_cap(n):
    """The termination guard's bound on nearest-neighbour searches per call."""
    return 4 * n + 16


def finish(n, id_lo, id_hi, height):
    """Discovery order -> R's hclust components: (merge (n-1) x 2, height,
    order (1-based), n_repairs)."""
    m = max(n - 1, 0)
    h = np.array(height, dtype=np.float64)[:m].copy()
    repairs = 0
    for t in range(m):
        top = max([h[t]] + [h[c - n] for c in (int(id_lo[t]), int(id_hi[t])) if c >= n])
        if top > h[t]:                         # one repair per raised step
            h[t] = top
            repairs += 1
    perm = np.argsort(h, kind="stable")
    rank = np.empty(m, np.int64)
    rank[perm] = np.arange(m)
    merge = np.zeros((m, 2), np.int32)
    for s in range(m):
        t = int(perm[s])
        row = [-(c + 1) if c < n else int(rank[c - n]) + 1 for c in (int(id_lo[t]), int(id_hi[t]))]
        x, y = row
        if x < 0 and y < 0:
            row = [max(x, y), min(x, y)]       # increasing node index
        else:
            row = [min(x, y), max(x, y)]       # a singleton first; two clusters by step
        merge[s] = row
    order = []
    todo = [m] if m else [-1]
    while todo:
        c = todo.pop()
        if c < 0:
            order.append(-c)
        else:
            todo.append(int(merge[c - 1, 1]))
            todo.append(int(merge[c - 1, 0]))
    return merge, h[perm], np.array(order, np.int32), repairs


def cutree_static(n, merge, height, cut_height, min_size):
    """WGCNA's cutreeStatic as the header states it: labels[n], 0 = unassigned."""
    member = [[i] for i in range(n)]           # leaves of singleton i / of step s at n + s
    top = list(range(n))                       # the current cluster of every node
    for s in range(max(n - 1, 0)):
        kids = [(-c - 1) if c < 0 else n + c - 1 for c in (int(merge[s, 0]), int(merge[s, 1]))]
        member.append(member[kids[0]] + member[kids[1]])
        if height[s] <= cut_height:
            for i in member[-1]:
                top[i] = n + s
    number, cut = {}, np.zeros(n, np.int64)
    for i in range(n):
        cut[i] = number.setdefault(top[i], len(number) + 1)
    sizes = np.bincount(cut, minlength=len(number) + 1)
    keep = [c for c in range(1, len(number) + 1) if sizes[c] >= min_size]
    keep.sort(key=lambda c: (-sizes[c], c))
    relabel = np.zeros(len(number) + 1, np.int32)
    for new, c in enumerate(keep):
        relabel[c] = new + 1
    return relabel[cut]


def clusters(n, children, heights):
    """{frozenset of leaves: height} of a tree given as rows (x, y) in
    construction order, ids 0 .. n-1 leaves and n + t the cluster of row t
    (scipy's Z[:, :2], or the chain's (id_lo, id_hi))."""
    leaves = [frozenset([i]) for i in range(n)]
    out = {}
    for t, (x, y) in enumerate(children):
        leaves.append(leaves[int(x)] | leaves[int(y)])
        out[leaves[-1]] = float(heights[t])
    return out


def clusters_of_merge(n, merge, heights):
    """The same of R's merge matrix (-(i + 1) singletons, s + 1 clusters)."""
    rows = [[(-c - 1) if c < 0 else n + c - 1 for c in (int(r[0]), int(r[1]))] for r in merge]
    return clusters(n, rows, heights)


def height_bar(n):
    """Relative bar on a height against another correct average linkage: a
    height is a size-weighted mean of up to n^2 / 4 original entries built by
    at most n - 1 nested convex combinations of non-negative terms, each adding
    a few ulps; (n + 16) 2^-52, the bar tests/tom_ref.py uses for sums of n
    terms."""
    return (n + 16) * 2.0 ** -52


def module_data(n, s, seed, n_factors=5, noise=0.6, layout_seed=None):
    """Module-structured data (s x n): n_factors latent factors, every node
    loading on one of them (contiguous blocks of unequal size, at least
    n / (2 n_factors) nodes each; drawn from layout_seed, by default seed) plus noise. Returns
    the data and the factor of every node."""
    lay = np.random.default_rng(seed if layout_seed is None else layout_seed)
    rng = np.random.default_rng([seed, 1])
    f = rng.standard_normal((s, n_factors))
    step = n // (2 * n_factors)
    cuts = np.cumsum(step + lay.multinomial(n - n_factors * step, np.ones(n_factors) / n_factors))[:-1]
    which = np.searchsorted(cuts, np.arange(n), side="right")
    x = f[:, which] * rng.uniform(0.7, 1.0, n) + noise * rng.standard_normal((s, n))
    return np.asfortranarray(x), which
