"""NetRep's Rcpp entry points, MI355X engine behind them.

Same names, argument meaning and return shapes as the functions registered in
src/RcppExports.cpp:131-146 (R wrappers R/RcppExports.R:4-35):

    Scale, CheckFinite, IntermediateProperties, IntermediatePropertiesNoData,
    PermutationProcedure, PermutationProcedureNoData, NetProps, NetPropsNoData

R values map to Python as:
  * ``NumericMatrix`` with dimnames -> ``RMatrix(values, rownames, colnames)``
    (``values`` an ``(nrow, ncol)`` array),
  * named ``CharacterVector`` moduleAssignments -> ``{node name: label}``
    (insertion order = the R vector's order),
  * ``List`` -> ``dict``; numeric arrays -> numpy (R's column-major cube layout
    for ``nulls``).
Errors raise ``NetRepError`` where the reference raises an R error.
Each call goes through the C ABI (``netrep_*``) into HIP kernels; nothing is
computed on the CPU.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
import sys
from dataclasses import dataclass
from typing import Mapping, Optional, Sequence

import numpy as np

from . import _lib as L

STATNAMES = ["avg.weight", "coherence", "cor.cor", "cor.degree", "cor.contrib",
             "avg.cor", "avg.contrib"]                       # src/permutations.cpp:174-177
STATNAMES_NODATA = ["avg.weight", "cor.cor", "cor.degree", "avg.cor"]  # src/permutationsNoData.cpp:156-158

DEFAULT_SEED = 0x4E65745265703133  # "NetRep13"


@dataclass
class RMatrix:
    """An R numeric matrix with dimnames."""
    values: np.ndarray
    rownames: Optional[Sequence[str]] = None
    colnames: Optional[Sequence[str]] = None

    @property
    def f(self) -> np.ndarray:
        return np.asfortranarray(np.asarray(self.values, dtype=np.float64))


_STRV_CACHE: "OrderedDict[tuple, tuple]" = OrderedDict()


def _strv(names: Sequence[str]):
    """A char** of `names` (and the bytes it points into). The last few name
    lists are kept: modulePreservation passes the same node names and module
    assignments on every call (C5: 100k strings, ~60 ms to re-encode)."""
    key = tuple(str(n) for n in names)
    hit = _STRV_CACHE.get(key)
    if hit is not None:
        _STRV_CACHE.move_to_end(key)
        return hit
    enc = [n.encode() for n in key]
    arr = (C.c_char_p * max(len(enc), 1))(*enc)
    _STRV_CACHE[key] = (arr, enc)
    while len(_STRV_CACHE) > 8:
        _STRV_CACHE.popitem(last=False)
    return arr, enc


def _assignments(module_assignments):
    if isinstance(module_assignments, Mapping):
        items = list(module_assignments.items())
    else:
        items = list(module_assignments)
    names = [str(n) for n, _ in items]
    labels = [str(lab) for _, lab in items]
    return names, labels


def _dptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def Scale(data) -> RMatrix:
    """Scale (src/scale.cpp:38-45): per-column (x - mean) / sd, keeping dimnames."""
    m = data if isinstance(data, RMatrix) else RMatrix(np.asarray(data))
    x = m.f
    out = np.empty_like(x, order="F")
    L.check_api(L.load().netrep_Scale(_dptr(x), x.shape[0], x.shape[1], _dptr(out)))
    return RMatrix(out, m.rownames, m.colnames)


def CheckFinite(mat) -> None:
    """CheckFinite (src/checkFinite.cpp:21-28): raise on any NA/NaN/Inf."""
    x = (mat.f if isinstance(mat, RMatrix) else np.asfortranarray(np.asarray(mat, dtype=np.float64)))
    x2 = x.reshape(x.shape[0], -1) if x.ndim > 1 else x.reshape(-1, 1)
    L.check_api(L.load().netrep_CheckFinite(_dptr(x2), x2.shape[0], x2.shape[1]))


class _IntermediateCall:
    """The module arguments and output buffers of an IntermediateProperties
    entry (``args``: from t_node_names to contribution_len, in the C order),
    and the unpacking of what the call wrote."""

    def __init__(self, t_node_names, module_assignments, modules, with_data):
        names, labels = _assignments(module_assignments)
        self.modules = [str(m) for m in modules]
        self.with_data = with_data
        t_node_names = list(t_node_names)
        # upper bounds for the concatenated outputs: module sizes in discovery
        sizes = {}
        tset = set(map(str, t_node_names))
        for nm, lab in zip(names, labels):
            if nm in tset:
                sizes[lab] = sizes.get(lab, 0) + 1
        ks = [sizes.get(m, 0) for m in self.modules]
        self.deg = np.empty(max(sum(ks), 1))
        self.cv = np.empty(max(sum(k * (k - 1) // 2 for k in ks), 1))
        self.nc = np.empty(max(sum(ks), 1)) if with_data else None
        nm_ = len(self.modules)
        self.deg_len = np.zeros(nm_, dtype=np.int64)
        self.cv_len = np.zeros(nm_, dtype=np.int64)
        self.nc_len = np.zeros(nm_, dtype=np.int64)
        tn, _k2 = _strv(t_node_names)
        an, _k3 = _strv(names)
        al, _k4 = _strv(labels)
        mo, _k5 = _strv(self.modules)
        self._keep = (_k2, _k3, _k4, _k5)
        i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
        self.args = (tn, len(t_node_names), an, al, len(names), mo, nm_, _dptr(self.deg), i64(self.deg_len),
                     _dptr(self.cv), i64(self.cv_len), _dptr(self.nc),
                     i64(self.nc_len) if self.nc is not None else None)

    def result(self) -> dict:
        out = {"degree": {}, "corr": {}}
        if self.with_data:
            out["contribution"] = {}
        od = oc = 0
        for i, m in enumerate(self.modules):
            if self.deg_len[i] == 0:
                continue                                     # only modsPresent (src/discProps.cpp:123-125)
            out["degree"][m] = self.deg[od:od + self.deg_len[i]].copy()
            out["corr"][m] = self.cv[oc:oc + self.cv_len[i]].copy()
            if self.with_data:
                out["contribution"][m] = self.nc[od:od + self.nc_len[i]].copy()
            od += self.deg_len[i]
            oc += self.cv_len[i]
        return out


def _intermediate(d_data, d_corr, d_net, t_node_names, module_assignments, modules):
    lib = L.load()
    d_names = list(d_net.colnames)
    n = len(d_names)
    corr = d_corr.f
    net = d_net.f
    data = d_data.f if d_data is not None else None
    s = data.shape[0] if data is not None else 0
    call = _IntermediateCall(t_node_names, module_assignments, modules, data is not None)
    dn, _k1 = _strv(d_names)
    L.check_api(lib.netrep_IntermediateProperties(_dptr(data), _dptr(corr), _dptr(net), s, n, dn, *call.args))
    return call.result()


def IntermediateProperties(dData: RMatrix, dCorr: RMatrix, dNet: RMatrix, tNodeNames,
                           moduleAssignments, modules) -> dict:
    """IntermediateProperties (src/discProps.cpp:44-132). dData must be scaled."""
    return _intermediate(dData, dCorr, dNet, list(tNodeNames), moduleAssignments, modules)


def IntermediatePropertiesNoData(dCorr: RMatrix, dNet: RMatrix, tNodeNames, moduleAssignments,
                                 modules) -> dict:
    """IntermediatePropertiesNoData (src/discProps.cpp:171-244)."""
    return _intermediate(None, dCorr, dNet, list(tNodeNames), moduleAssignments, modules)


def _null_pool_size(ma_names, t_names, null_hypothesis) -> int:
    """|nullIdx| of MakeNullMap (src/utils.cpp:108-136) over validNodes
    (src/permutations.cpp:319-323)."""
    tset = set(t_names)
    if str(null_hypothesis) == "all":
        return len(tset)
    return len({nm for nm in ma_names if nm in tset})


_hook_keep = None


def set_interrupt_hook(fn) -> None:
    """Install ``fn() -> bool`` as the interrupt check polled (every 100 ms) by
    PermutationProcedure while the GPUs work (checkInterrupt,
    src/interrupt.cpp:9-11, in MonitorProgress, src/thread-utils.cpp:49-82).
    A true return cancels the run; the call then returns the partial cube
    (un-run permutations NA) with ``res["interrupted"] = True``. ``None``
    removes the hook."""
    global _hook_keep
    lib = L.load()
    if fn is None:
        lib.netrep_set_interrupt_hook(None, None)
        _hook_keep = None
        return
    cb = L.INTERRUPT_FN(lambda _user: 1 if fn() else 0)
    _hook_keep = cb
    lib.netrep_set_interrupt_hook(C.cast(cb, C.c_void_p), None)


_progress_keep = None
_progress_user_set = False


def format_progress(done: int, total: int) -> str:
    """MonitorProgress's line, "\\r%5d% completed." (src/thread-utils.cpp:66-68),
    rendered by the library (netrep_format_progress)."""
    buf = C.create_string_buffer(64)
    n = L.load().netrep_format_progress(int(done), int(total), buf, 64)
    return buf.value.decode() if n >= 0 else ""


def _install_progress(fn) -> None:
    global _progress_keep
    lib = L.load()
    if fn is None:
        lib.netrep_set_progress_hook(None, None)
        _progress_keep = None
        return
    cb = L.PROGRESS_FN(lambda ev, done, total, _user: fn(int(ev), int(done), int(total)))
    _progress_keep = cb
    lib.netrep_set_progress_hook(C.cast(cb, C.c_void_p), None)


def set_progress_hook(fn) -> None:
    """Install ``fn(event, done, total)`` as the progress report of a verbose
    PermutationProcedure (netrep_set_progress_hook; event 0 begin, 1 update
    about once a second, 2 end) -- MonitorProgress's console output
    (src/thread-utils.cpp:54-81). ``None`` restores the default, which prints
    the reference's lines to ``sys.stdout``; the library itself never writes
    to stdout."""
    global _progress_user_set
    _progress_user_set = fn is not None
    _install_progress(fn)


def _print_progress(ev: int, done: int, total: int) -> None:
    if ev == L.PROGRESS_BEGIN:
        sys.stdout.write("\n")
    elif ev == L.PROGRESS_UPDATE:
        sys.stdout.write(format_progress(done, total))
    else:
        sys.stdout.write("\n\n")
    sys.stdout.flush()


# Datasets handed to netrep_PrefetchTestDataset: their column-major arrays
# stay referenced here until the PermutationProcedure call that adopts them
# (at most two pending, as in the library).
_prefetched = []


def _prefetch_key(t_data, t_corr, t_net):
    return (id(t_data.values) if t_data is not None else None, id(t_corr.values), id(t_net.values))


def PrefetchTestDataset(tData: Optional[RMatrix], tCorr: RMatrix, tNet: RMatrix) -> None:
    """Start uploading a later test dataset to the GPU in the background
    (netrep_PrefetchTestDataset), so that its host->HBM copy overlaps the
    permutations of the current one -- modulePreservation's loop over test
    datasets (R/modulePreservation.R:553-620): prefetch dataset t+1, then run
    dataset t. The PermutationProcedure call on these same matrices adopts
    the upload."""
    lib = L.load()
    corr, net = tCorr.f, tNet.f
    data = tData.f if tData is not None else None
    s = data.shape[0] if data is not None else 0
    rc = lib.netrep_PrefetchTestDataset(_dptr(data), _dptr(corr), _dptr(net), s, corr.shape[0])
    L.check_api(rc)
    _prefetched.append((_prefetch_key(tData, tCorr, tNet), (data, corr, net), (tData, tCorr, tNet)))
    del _prefetched[:-2]


def DiscardPrefetch() -> None:
    """Drop every pending PrefetchTestDataset upload (netrep_DiscardPrefetch)."""
    L.load().netrep_DiscardPrefetch()
    _prefetched.clear()


def ReleaseResident() -> None:
    """Free the datasets kept resident between calls (IntermediateProperties'
    discovery dataset, NetProps' dataset), pending prefetches and the pooled
    contexts (netrep_ReleaseResident; the R glue calls it when
    modulePreservation / networkProperties return)."""
    L.load().netrep_ReleaseResident()
    _prefetched.clear()


def h2d_bytes() -> int:
    """Host -> device bytes the library has copied since it was loaded
    (nr_h2d_bytes): the difference across calls shows what was uploaded."""
    v = C.c_int64()
    L.check(L.load().nr_h2d_bytes(C.byref(v)))
    return int(v.value)


def _marshal_disc_props(disc_props, modules, with_data):
    """netrep_disc_props of a discProps dict ({"degree" | "corr" | "contribution":
    {module: vector}}) in `modules` order, and the arrays its pointers refer to
    (keep them alive across the call)."""
    nm_ = len(modules)
    keep = []

    def vecs(key):
        d = disc_props.get(key, {}) if disc_props is not None else {}
        ptrs = (C.POINTER(C.c_double) * max(nm_, 1))()
        lens = np.zeros(max(nm_, 1), dtype=np.int64)
        for i, m in enumerate(modules):
            if m in d:
                v = np.ascontiguousarray(d[m], dtype=np.float64)
                keep.append(v)
                ptrs[i] = _dptr(v)
                lens[i] = v.size
        keep.append(lens)
        return ptrs, lens.ctypes.data_as(C.POINTER(C.c_int64))

    dp = L.DiscProps()
    dp.degree, dp.degree_len = vecs("degree")
    dp.corr, dp.corr_len = vecs("corr")
    if with_data:
        dp.contribution, dp.contribution_len = vecs("contribution")
    return dp, keep


def _permutation_result(rc, modules, with_data, observed, nulls, n_perm):
    """The PermutationProcedure list of an entry's return code and outputs; an
    interrupted run returns the partial, NA-padded cube
    (src/permutations.cpp:375-408)."""
    interrupted = rc == L.NR_ERR_CANCELLED
    if not interrupted:
        L.check_api(rc)
    statnames = STATNAMES if with_data else STATNAMES_NODATA
    res = {"observed": observed, "observed_dimnames": (modules, statnames)}
    if interrupted:
        res["interrupted"] = True
    if n_perm > 0:
        res["nulls"] = nulls
        res["nulls_dimnames"] = (modules, statnames, None)  # "permutation.i" left implicit
    return res


def _permutation(disc_props, t_data, t_corr, t_net, module_assignments, modules, n_perm, n_cores,
                 null_hypothesis, verbose, seed, pi):
    lib = L.load()
    names, labels = _assignments(module_assignments)
    modules = [str(m) for m in modules]
    with_data = t_data is not None
    t_names = list(t_net.colnames)
    n = len(t_names)
    key = _prefetch_key(t_data, t_corr, t_net)
    pre = next((p for p in _prefetched if p[0] == key), None)
    if pre is not None:
        _prefetched.remove(pre)
        data, corr, net = pre[1]   # the very arrays the upload read (same pointers)
    else:
        corr, net = t_corr.f, t_net.f
        data = t_data.f if with_data else None
    s = data.shape[0] if with_data else 0
    nm_ = len(modules)
    dp, _keep = _marshal_disc_props(disc_props, modules, with_data)
    n_stat = 7 if with_data else 4
    observed = np.empty((nm_, n_stat), order="F")
    nulls = np.empty((nm_, n_stat, int(n_perm)), order="F") if n_perm > 0 else None
    pi_arr = None
    if pi is not None:
        pi_arr = np.ascontiguousarray(pi, dtype=np.uint32)
        n_null = _null_pool_size(names, t_names, null_hypothesis)
        if pi_arr.ndim != 2 or pi_arr.shape != (int(n_perm), n_null):
            raise L.NetRepError(L.NR_ERR_INVALID, f"pi must have shape (nPermutations, n_null) = "
                                                  f"({int(n_perm)}, {n_null}), got {pi_arr.shape}")
    tn, _k1 = _strv(t_names)
    an, _k2 = _strv(names)
    al, _k3 = _strv(labels)
    mo, _k4 = _strv(modules)
    if verbose and not _progress_user_set:
        _install_progress(_print_progress)  # the reference's console lines, from Python
    rc = lib.netrep_PermutationProcedure(
        C.byref(dp), _dptr(data), _dptr(corr), _dptr(net), s, n, tn, an, al, len(names), mo, nm_,
        int(n_perm), int(n_cores), str(null_hypothesis).encode(), int(bool(verbose)),
        int(seed) & (2**64 - 1), pi_arr.ctypes.data_as(C.POINTER(C.c_uint32)) if pi_arr is not None else None,
        _dptr(nulls), _dptr(observed))
    return _permutation_result(rc, modules, with_data, observed, nulls, n_perm)


def PermutationProcedure(discProps: dict, tData: RMatrix, tCorr: RMatrix, tNet: RMatrix,
                         moduleAssignments, modules, nPermutations: int, nCores: int = 1,
                         nullHypothesis: str = "overlap", verbose: bool = False,
                         seed: int = DEFAULT_SEED, pi=None) -> dict:
    """PermutationProcedure (src/permutations.cpp:160-409).

    Returns ``{"nulls": (M, 7, P), "observed": (M, 7)}`` (plus dimnames).
    ``seed`` keys the per-permutation shuffle; ``pi`` ((P, n_null) uint32)
    replaces it with explicit shuffles of the null pool.
    """
    return _permutation(discProps, tData, tCorr, tNet, moduleAssignments, modules, nPermutations,
                        nCores, nullHypothesis, verbose, seed, pi)


def read_rds_matrix(path: str, object: Optional[str] = None) -> RMatrix:
    """One numeric matrix from an RDS file (saveRDS, gzip or uncompressed) or,
    by name, a save() archive -- what disk.matrix holds
    (R/disk-matrix-class.R:175-182) -- via netrep_ReadRDSMatrix (host read)."""
    lib = L.load()
    nrow, ncol, need = C.c_int64(), C.c_int64(), C.c_int64()
    p = str(path).encode()
    o = None if object is None else str(object).encode()
    L.check_api(lib.netrep_ReadRDSMatrix(p, o, C.byref(nrow), C.byref(ncol), None, None, 0, C.byref(need)))
    out = np.empty((nrow.value, ncol.value), order="F")
    buf = C.create_string_buffer(max(need.value, 1))
    L.check_api(lib.netrep_ReadRDSMatrix(p, o, C.byref(nrow), C.byref(ncol), _dptr(out), buf, need.value,
                                         C.byref(need)))
    names = [x.decode() for x in buf.raw[:need.value].split(b"\0")[:-1]] if need.value else None
    return RMatrix(out, None, names)


def PermutationProcedureFiles(discProps: dict, tData_file: Optional[str], tCorr_file: str, tNet_file: str,
                              moduleAssignments, modules, nPermutations: int, nCores: int = 1,
                              nullHypothesis: str = "overlap", verbose: bool = False,
                              seed: int = DEFAULT_SEED, pi=None) -> dict:
    """PermutationProcedure[NoData] on a test dataset held as disk.matrix files
    (netrep_PermutationProcedureFiles): the files go straight to HBM and tData
    (raw, unscaled) is scaled on the device; node names are the network file's
    column names."""
    lib = L.load()
    names, labels = _assignments(moduleAssignments)
    modules = [str(m) for m in modules]
    with_data = tData_file is not None
    nm_ = len(modules)
    dp, _keep = _marshal_disc_props(discProps, modules, with_data)
    n_stat = 7 if with_data else 4
    observed = np.empty((nm_, n_stat), order="F")
    nulls = np.empty((nm_, n_stat, int(nPermutations)), order="F") if nPermutations > 0 else None
    pi_arr = None if pi is None else np.ascontiguousarray(pi, dtype=np.uint32)
    an, _k2 = _strv(names)
    al, _k3 = _strv(labels)
    mo, _k4 = _strv(modules)
    enc = lambda x: None if x is None else str(x).encode()  # noqa: E731
    if pi_arr is not None and (pi_arr.ndim != 2 or pi_arr.shape[0] != int(nPermutations)):
        raise L.NetRepError(L.NR_ERR_INVALID, f"pi must have shape (nPermutations, n_null), got {pi_arr.shape}")
    if verbose and not _progress_user_set:
        _install_progress(_print_progress)
    # n_null is known only once the files' node names are read: the library
    # checks pi's length against it (pi_len)
    rc = lib.netrep_PermutationProcedureFiles(
        C.byref(dp), enc(tData_file), enc(tCorr_file), enc(tNet_file), an, al, len(names), mo, nm_,
        int(nPermutations), int(nCores), str(nullHypothesis).encode(), int(bool(verbose)),
        int(seed) & (2**64 - 1), pi_arr.ctypes.data_as(C.POINTER(C.c_uint32)) if pi_arr is not None else None,
        int(pi_arr.size) if pi_arr is not None else -1, _dptr(nulls), _dptr(observed))
    return _permutation_result(rc, modules, with_data, observed, nulls, nPermutations)


def _named_data(data, what):
    """(node names, column-major values) of a from-data entry's data matrix."""
    if getattr(data, "colnames", None) is None:
        raise L.NetRepError(L.NR_ERR_INVALID, f"{what} needs colnames (the node names)")
    names = [str(n) for n in data.colnames]
    x = data.f
    if x.ndim != 2 or len(names) != x.shape[1]:
        raise L.NetRepError(L.NR_ERR_INVALID, f"{what} must have one colname per column")
    return names, x


class _DataPermutationCall:
    """The arguments after the dataset of a permutation entry whose test
    dataset has data and is named by ``t_names`` (``args``: from ma_names to
    observed_out, in the C order), and the result of the call."""

    def __init__(self, disc_props, t_names, module_assignments, modules, n_perm, n_cores, null_hypothesis,
                 verbose, seed, pi):
        names, labels = _assignments(module_assignments)
        self.modules = [str(m) for m in modules]
        self.n_perm = int(n_perm)
        nm_ = len(self.modules)
        self.dp, self._keep = _marshal_disc_props(disc_props, self.modules, True)
        self.observed = np.empty((nm_, 7), order="F")
        self.nulls = np.empty((nm_, 7, self.n_perm), order="F") if self.n_perm > 0 else None
        pi_arr = None
        if pi is not None:
            pi_arr = np.ascontiguousarray(pi, dtype=np.uint32)
            n_null = _null_pool_size(names, t_names, null_hypothesis)
            if pi_arr.ndim != 2 or pi_arr.shape != (self.n_perm, n_null):
                raise L.NetRepError(L.NR_ERR_INVALID, f"pi must have shape (nPermutations, n_null) = "
                                                      f"({self.n_perm}, {n_null}), got {pi_arr.shape}")
        self._pi = pi_arr
        an, _k2 = _strv(names)
        al, _k3 = _strv(labels)
        mo, _k4 = _strv(self.modules)
        self._strs = (_k2, _k3, _k4)
        if verbose and not _progress_user_set:
            _install_progress(_print_progress)
        self.args = (an, al, len(names), mo, nm_, self.n_perm, int(n_cores), str(null_hypothesis).encode(),
                     int(bool(verbose)), int(seed) & (2**64 - 1),
                     pi_arr.ctypes.data_as(C.POINTER(C.c_uint32)) if pi_arr is not None else None,
                     _dptr(self.nulls), _dptr(self.observed))

    def result(self, rc) -> dict:
        return _permutation_result(rc, self.modules, True, self.observed, self.nulls, self.n_perm)


def PermutationProcedureFromData(discProps: dict, tData: RMatrix, beta: float, moduleAssignments, modules,
                                 nPermutations: int, nCores: int = 1, nullHypothesis: str = "overlap",
                                 verbose: bool = False, seed: int = DEFAULT_SEED, pi=None,
                                 networkType: str = "unsigned", scaleData: bool = False,
                                 tom: bool = False, corType: str = "pearson") -> dict:
    """PermutationProcedure on a test dataset given as its data matrix alone
    (netrep_PermutationProcedureFromData): ``tData`` (samples x nodes, its
    colnames the node names; scaled already unless ``scaleData``) is the only
    upload, and the test correlation (cor(tData)) and network (``networkType``
    'unsigned' |cor|^beta, 'signed' ((1 + cor) / 2)^beta, 'signed_hybrid'
    cor^beta where cor > 0, else 0; with ``tom=True`` the topological overlap
    matrix of that adjacency, WGCNA's unsigned TOM with TOMDenom "min") are
    built on the GPU. ``corType`` 'spearman' or 'bicor' (WGCNA's bicor with
    its defaults): the correlation is of that type, computed on the GPU from
    the resident scaled data, which stay what the data statistics (coherence,
    cor.contrib, avg.contrib) are computed from. Raises
    ``NetRepError`` (``NR_ERR_NONFINITE``) if they are not all finite, e.g.
    for a constant column."""
    lib = L.load()
    t_names, data = _named_data(tData, "tData")
    s, n = data.shape
    call = _DataPermutationCall(discProps, t_names, moduleAssignments, modules, nPermutations, nCores,
                                nullHypothesis, verbose, seed, pi)
    tn, _k1 = _strv(t_names)
    rc = lib.netrep_PermutationProcedureFromData(
        C.byref(call.dp), _dptr(data), int(bool(scaleData)), L.net_type_code(networkType, tom, corType),
        float(beta), s, n, tn, *call.args)
    return call.result(rc)


def BuildNetwork(data, beta: float, networkType: str = "unsigned", scaleData: bool = True, tom: bool = False,
                 corType: str = "pearson"):
    """(correlation, network) of a data matrix, built on the GPU as the from-data
    path builds them (netrep_BuildNetwork) and copied back, for callers who
    still need host matrices (the discovery-side calls have a from-data route
    of their own: FromDataDataset, IntermediatePropertiesFromData). ``data`` is raw
    unless ``scaleData=False``. ``tom=True``: the network returned is the
    topological overlap matrix of the adjacency. ``corType`` 'spearman' or
    'bicor': the correlation returned is Spearman's or WGCNA's biweight
    midcorrelation (and the network is built from it). Node names: the data's
    colnames."""
    m = data if isinstance(data, RMatrix) else RMatrix(np.asarray(data))
    x = m.f
    s, n = x.shape
    corr = np.empty((n, n), order="F")
    net = np.empty((n, n), order="F")
    L.check_api(L.load().netrep_BuildNetwork(_dptr(x), int(bool(scaleData)),
                                             L.net_type_code(networkType, tom, corType),
                                             float(beta), s, n, _dptr(corr), _dptr(net)))
    return RMatrix(corr, m.colnames, m.colnames), RMatrix(net, m.colnames, m.colnames)


# pickSoftThreshold's default powerVector: c(1:10, seq(12, 20, by = 2))
DEFAULT_POWERS = tuple(range(1, 11)) + tuple(range(12, 21, 2))
# the columns of its fitIndices table, in order
SFT_COLUMNS = ["Power", "SFT.R.sq", "slope", "truncated.R.sq", "mean.k.", "median.k.", "max.k."]


def ScaleFreeFit(k, nBreaks: int = 10, removeFirst: bool = False) -> dict:
    """WGCNA's scaleFreeFitIndex of one connectivity vector (netrep_ScaleFreeFit;
    host only, no GPU): ``{"Rsquared.SFT", "slope.SFT", "truncatedExponentialAdjRsquared"}``.
    All NaN for a constant or non-finite ``k``."""
    v = np.ascontiguousarray(k, dtype=np.float64).ravel()
    out = np.empty(3)
    L.check_api(L.load().netrep_ScaleFreeFit(_dptr(v), v.size, int(nBreaks), int(bool(removeFirst)), _dptr(out)))
    return {"Rsquared.SFT": float(out[0]), "slope.SFT": float(out[1]),
            "truncatedExponentialAdjRsquared": float(out[2])}


def PickSoftThreshold(data, powerVector=DEFAULT_POWERS, networkType: str = "unsigned", corType: str = "pearson",
                      scaleData: bool = True, RsquaredCut: float = 0.85, nBreaks: int = 10,
                      removeFirst: bool = False, returnConnectivity: bool = False) -> dict:
    """WGCNA's pickSoftThreshold from the data matrix alone
    (netrep_PickSoftThreshold): ``data`` (samples x nodes, raw unless
    ``scaleData=False``) is the only upload; the connectivities of every
    candidate power are summed on the GPU without an n x n matrix anywhere,
    and the scale-free fit of each runs on the host. Returns
    ``{"powerEstimate": the first power with -sign(slope) SFT.R.sq >
    RsquaredCut or None, "fitIndices": {column: array}}`` (columns
    ``SFT_COLUMNS``), plus ``"connectivity"`` (nodes x powers) with
    ``returnConnectivity``. Raises ``NetRepError`` (``NR_ERR_NONFINITE``) for
    a constant column."""
    m = data if isinstance(data, RMatrix) else RMatrix(np.asarray(data))
    x = m.f
    if x.ndim != 2:
        raise L.NetRepError(L.NR_ERR_INVALID, "data must be a samples x nodes matrix")
    s, n = x.shape
    p = np.ascontiguousarray(np.atleast_1d(powerVector), dtype=np.float64)
    if p.ndim != 1:
        raise L.NetRepError(L.NR_ERR_INVALID, "powerVector must be a vector")
    table = np.empty((p.size, len(SFT_COLUMNS)), order="F")
    est = C.c_double()
    k = np.empty((n, p.size), order="F") if returnConnectivity else None
    L.check_api(L.load().netrep_PickSoftThreshold(
        _dptr(x), int(bool(scaleData)), L.net_type_code(networkType, False, corType), s, n, _dptr(p), int(p.size),
        float(RsquaredCut), int(nBreaks), int(bool(removeFirst)), _dptr(table), C.cast(C.byref(est), L._dp),
        _dptr(k)))
    out = {"powerEstimate": None if np.isnan(est.value) else float(est.value),
           "fitIndices": {c: table[:, i].copy() for i, c in enumerate(SFT_COLUMNS)}}
    if returnConnectivity:
        out["connectivity"] = k
    return out


def PermutationProcedureNoData(discProps: dict, tCorr: RMatrix, tNet: RMatrix, moduleAssignments,
                               modules, nPermutations: int, nCores: int = 1,
                               nullHypothesis: str = "overlap", verbose: bool = False,
                               seed: int = DEFAULT_SEED, pi=None) -> dict:
    """PermutationProcedureNoData (src/permutationsNoData.cpp:140-375)."""
    return _permutation(discProps, None, tCorr, tNet, moduleAssignments, modules, nPermutations,
                        nCores, nullHypothesis, verbose, seed, pi)


class _NetPropsCall:
    """The module arguments and output buffers of a NetProps entry (``args``:
    from ma_names to k_all_out, in the C order) for a dataset of ``s`` samples
    (0: no data), and the unpacking of what the call wrote."""

    def __init__(self, module_assignments, modules, s, with_data):
        self.names, self.labels = _assignments(module_assignments)
        self.modules = [str(m) for m in modules]
        self.s, self.with_data = s, with_data
        k_all = {}
        for lab in self.labels:
            k_all[lab] = k_all.get(lab, 0) + 1
        tot = sum(k_all.get(m, 0) for m in self.modules)
        nm_ = len(self.modules)
        self.deg = np.empty(max(tot, 1))
        self.aw = np.empty(max(nm_, 1))
        self.kk = np.zeros(max(nm_, 1), dtype=np.int64)
        self.nc = np.empty(max(tot, 1)) if with_data else None
        self.sp = np.empty(max(nm_ * s, 1)) if with_data else None
        self.coh = np.empty(max(nm_, 1)) if with_data else None
        an, _k2 = _strv(self.names)
        al, _k3 = _strv(self.labels)
        mo, _k4 = _strv(self.modules)
        self._keep = (_k2, _k3, _k4)
        self.args = (an, al, len(self.names), mo, nm_, _dptr(self.deg), _dptr(self.nc), _dptr(self.sp),
                     _dptr(self.coh), _dptr(self.aw), self.kk.ctypes.data_as(C.POINTER(C.c_int64)))

    def result(self) -> dict:
        mod_nodes = {}
        for nm, lab in zip(self.names, self.labels):
            mod_nodes.setdefault(lab, []).append(nm)
        res = {}
        o = 0
        s = self.s
        for i, m in enumerate(self.modules):
            k = int(self.kk[i])
            entry = {"degree": self.deg[o:o + k].copy(), "avgWeight": float(self.aw[i]),
                     "node_names": mod_nodes.get(m, [])}
            if self.with_data:
                entry.update(summary=self.sp[i * s:(i + 1) * s].copy(), contribution=self.nc[o:o + k].copy(),
                             coherence=float(self.coh[i]))
            res[m] = entry
            o += k
        return res


def _netprops(data, net, module_assignments, modules):
    lib = L.load()
    node_names = list(net.colnames)
    netv = net.f
    x = data.f if data is not None else None
    s = x.shape[0] if x is not None else 0
    call = _NetPropsCall(module_assignments, modules, s, x is not None)
    nn, _k1 = _strv(node_names)
    L.check_api(lib.netrep_NetProps(_dptr(x), _dptr(netv), s, len(node_names), nn, *call.args))
    return call.result()


def NetProps(data: RMatrix, net: RMatrix, moduleAssignments, modules) -> dict:
    """NetProps (src/properties.cpp:41-156). ``data`` is unscaled; it is scaled on the GPU."""
    return _netprops(data, net, moduleAssignments, modules)


def NetPropsNoData(net: RMatrix, moduleAssignments, modules) -> dict:
    """NetPropsNoData (src/properties.cpp:190-273)."""
    return _netprops(None, net, moduleAssignments, modules)


class FromDataDataset:
    """A dataset built on the GPU from its data matrix alone and kept there
    (netrep_DatasetFromData), to be used in every role without another upload
    or build: the discovery side (``intermediate_properties``), network
    properties (``net_props``) and the test side (``permutation_procedure``).
    ``data`` (samples x nodes, its colnames the node names; raw unless
    ``scaleData=False``) is the only upload; ``beta``, ``networkType``, ``tom``
    and ``corType`` as in PermutationProcedureFromData. Raises ``NetRepError``
    (``NR_ERR_NONFINITE``) for a constant column. A context manager;
    ``close()`` frees the device memory (ReleaseResident does not). After
    ``close()`` every method raises ``NetRepError`` (``NR_ERR_INVALID``)."""

    def __init__(self, data: RMatrix, beta: float, networkType: str = "unsigned", scaleData: bool = True,
                 tom: bool = False, corType: str = "pearson", nCores: int = 0):
        self._h = None
        lib = L.load()
        self.node_names, x = _named_data(data, "data")
        self.n_samples, self.n_nodes = x.shape
        nn, _k1 = _strv(self.node_names)
        h = C.c_void_p()
        L.check_api(lib.netrep_DatasetFromData(_dptr(x), int(bool(scaleData)), L.net_type_code(networkType, tom, corType),
                                               float(beta), self.n_samples, self.n_nodes, nn, int(nCores),
                                               C.byref(h)))
        self._h = h

    def _handle(self):
        if self._h is None:
            raise L.NetRepError(L.NR_ERR_INVALID, "the dataset is closed")
        return self._h

    def close(self) -> None:
        h, self._h = self._h, None
        if h is not None:
            L.load().netrep_DatasetRelease(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass

    def intermediate_properties(self, tNodeNames, moduleAssignments, modules) -> dict:
        """IntermediateProperties with this dataset as the discovery dataset."""
        h = self._handle()
        call = _IntermediateCall(tNodeNames, moduleAssignments, modules, True)
        L.check_api(L.load().netrep_DatasetIntermediateProperties(h, *call.args))
        return call.result()

    def net_props(self, moduleAssignments, modules) -> dict:
        """NetProps of this dataset's network and (scaled) data."""
        h = self._handle()
        call = _NetPropsCall(moduleAssignments, modules, self.n_samples, True)
        L.check_api(L.load().netrep_DatasetNetProps(h, *call.args))
        return call.result()

    def permutation_procedure(self, discProps: dict, moduleAssignments, modules, nPermutations: int,
                              nCores: int = 1, nullHypothesis: str = "overlap", verbose: bool = False,
                              seed: int = DEFAULT_SEED, pi=None) -> dict:
        """PermutationProcedureFromData with this dataset as the test dataset;
        the dataset stays resident and unchanged."""
        h = self._handle()
        call = _DataPermutationCall(discProps, self.node_names, moduleAssignments, modules, nPermutations, nCores,
                                    nullHypothesis, verbose, seed, pi)
        rc = L.load().netrep_DatasetPermutationProcedure(C.byref(call.dp), h, *call.args)
        return call.result(rc)

    def matrices(self):
        """(correlation, network) copied back, as BuildNetwork returns them."""
        h = self._handle()
        n = self.n_nodes
        corr = np.empty((n, n), order="F")
        net = np.empty((n, n), order="F")
        L.check_api(L.load().netrep_DatasetMatrices(h, _dptr(corr), _dptr(net)))
        return RMatrix(corr, self.node_names, self.node_names), RMatrix(net, self.node_names, self.node_names)

    def hclust(self) -> dict:
        """The average-linkage gene dendrogram of this dataset's network on
        d = 1 - net (netrep_DatasetHclust), built on the GPU, as the
        components of R's ``hclust`` object: ``merge`` ((n - 1) x 2),
        ``height``, ``order`` (1-based), ``labels`` (the node names),
        ``method`` "average"; ``n_repairs`` beside them. The dataset stays
        resident and unchanged."""
        h = self._handle()
        n = self.n_nodes
        merge = np.zeros((max(n - 1, 0), 2), dtype=np.int32, order="F")
        height = np.zeros(max(n - 1, 0), dtype=np.float64)
        order = np.zeros(n, dtype=np.int32)
        repairs = C.c_int32()
        L.check_api(L.load().netrep_DatasetHclust(h, _i32ptr(merge), _dptr(height), _i32ptr(order), C.byref(repairs)))
        return {"merge": merge, "height": height, "order": order, "labels": list(self.node_names),
                "method": "average", "n_repairs": int(repairs.value)}


    # -- what follows a cut: eigengenes, membership, merging, trimming ------
    def _labels(self, labels) -> np.ndarray:
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        if lab.shape != (self.n_nodes,):
            raise L.NetRepError(L.NR_ERR_INVALID, "labels must hold one integer per node, in node order")
        return lab

    def module_eigengenes(self, labels) -> dict:
        """The eigengene of every module of ``labels`` (one integer per node
        in node order, 0 unassigned) on the GPU (netrep_DatasetModuleEigengenes):
        ``modules`` (the distinct positive labels, increasing), ``eigengenes``
        (S x M), ``varExplained`` (M) and ``kME`` (n: each node's correlation
        with its own module's eigengene, NaN for label 0). The eigengene is
        that of the resident data: WGCNA's ``moduleEigengenes`` for a handle
        built with ``scaleData=True``; with ``False`` it is the unscaled
        data's."""
        h = self._handle()
        lab = self._labels(labels)
        m = max(int(np.unique(lab[lab > 0]).size), 1)
        mods = np.zeros(m, dtype=np.int32)
        eig = np.zeros((self.n_samples, m), order="F")
        ve = np.zeros(m)
        own = np.zeros(self.n_nodes)
        n_mod = C.c_int32()
        L.check_api(L.load().netrep_DatasetModuleEigengenes(h, _i32ptr(lab), C.byref(n_mod), _i32ptr(mods), _dptr(eig),
                                                            _dptr(ve), _dptr(own)))
        return {"modules": mods, "eigengenes": eig, "varExplained": ve, "kME": own}

    def module_membership(self, labels) -> RMatrix:
        """The module-membership table kME, the correlation of every node
        with every module eigengene of ``labels``, computed on the GPU from
        the resident data (netrep_DatasetModuleMembership): n rows named by
        node, columns ``"kME<label>"``. Eigengenes as ``module_eigengenes``."""
        h = self._handle()
        lab = self._labels(labels)
        mods = np.unique(lab[lab > 0])
        kme = np.zeros((self.n_nodes, max(int(mods.size), 1)), order="F")
        L.check_api(L.load().netrep_DatasetModuleMembership(h, _i32ptr(lab), _dptr(kme)))
        return RMatrix(kme, list(self.node_names), [f"kME{int(m)}" for m in mods])

    def merge_close_modules(self, labels, cutHeight: float = 0.25, relabel: bool = True) -> dict:
        """WGCNA's ``mergeCloseModules`` (iterate = TRUE) on the handle
        (netrep_DatasetMergeCloseModules; include/netrep_gpu.h has the
        rules): modules whose eigengenes are closer than ``cutHeight`` on
        1 - cor in the average-linkage tree are merged, round after round,
        until a round merges nothing. ``labels`` the merged labels
        (renumbered 1, 2, ... by decreasing size with ``relabel``), ``rounds``
        the rounds that merged something, ``eigengenes`` (S x M') of the
        final modules in their label order, ``heights`` (M' - 1) of their
        tree."""
        h = self._handle()
        lab = self._labels(labels)
        m = max(int(np.unique(lab[lab > 0]).size), 1)
        out = np.zeros(self.n_nodes, dtype=np.int32)
        eig = np.zeros((self.n_samples, m), order="F")
        heights = np.zeros(max(m - 1, 1))
        rounds, m_last = C.c_int32(), C.c_int32()
        L.check_api(L.load().netrep_DatasetMergeCloseModules(h, _i32ptr(lab), float(cutHeight), int(bool(relabel)),
                                                             _i32ptr(out), C.byref(rounds), C.byref(m_last),
                                                             _dptr(eig), _dptr(heights)))
        ml = int(m_last.value)
        return {"labels": out, "rounds": int(rounds.value), "eigengenes": np.asfortranarray(eig[:, :ml]),
                "heights": heights[:max(ml - 1, 0)].copy()}

    def trim_modules(self, labels, minSize: int, minKMEtoStay: float = 0.3, minCoreKME: float = 0.5,
                     minCoreKMESize=None) -> np.ndarray:
        """The kME trimming of WGCNA's ``blockwiseModules``, in-module kME
        only (netrep_DatasetTrimModules): a module with fewer than
        ``minCoreKMESize`` (default ``minSize / 3``) nodes of kME above
        ``minCoreKME`` is dissolved, otherwise its nodes of kME below
        ``minKMEtoStay`` go to 0, and a module left under ``minSize`` nodes
        is dissolved. One pass, no relabelling; the reassignment by kME
        p-value (``reassignThreshold``) is not offered."""
        h = self._handle()
        lab = self._labels(labels)
        out = np.zeros(self.n_nodes, dtype=np.int32)
        core = -1 if minCoreKMESize is None else int(minCoreKMESize)
        L.check_api(L.load().netrep_DatasetTrimModules(h, _i32ptr(lab), float(minKMEtoStay), float(minCoreKME), core,
                                                       int(minSize), _i32ptr(out)))
        return out

    # -- connectivity by module: the table, hub nodes, node and sample order -
    def module_connectivity(self, labels):
        """The module-connectivity table, the network-side counterpart of
        ``module_membership``, computed on the GPU from the resident network
        (netrep_DatasetModuleConnectivity): ``(kMod, kTotal)``. ``kMod`` has n
        rows named by node and columns ``"k<label>"``: the summed weight of
        the node's edges into each module of ``labels`` (itself excluded);
        ``kTotal`` (n) the same over every other node, unassigned ones
        included."""
        h = self._handle()
        lab = self._labels(labels)
        mods = np.unique(lab[lab > 0])
        k_mod = np.zeros((self.n_nodes, max(int(mods.size), 1)), order="F")
        k_total = np.zeros(self.n_nodes)
        L.check_api(L.load().netrep_DatasetModuleConnectivity(h, _i32ptr(lab), _dptr(k_total), _dptr(k_mod)))
        return RMatrix(k_mod, list(self.node_names), [f"k{int(m)}" for m in mods]), k_total

    def intramodular_connectivity(self, labels) -> dict:
        """WGCNA's ``intramodularConnectivity`` on the handle's network
        (netrep_DatasetIntramodularConnectivity): ``kTotal``, ``kWithin`` (the
        node's connectivity to its own module), ``kOut = kTotal - kWithin``
        and ``kDiff = kWithin - kOut``, each of length n, the last three NaN
        for label 0; ``modules`` the distinct positive labels."""
        h = self._handle()
        lab = self._labels(labels)
        out = {k: np.zeros(self.n_nodes) for k in ("kTotal", "kWithin", "kOut", "kDiff")}
        L.check_api(L.load().netrep_DatasetIntramodularConnectivity(h, _i32ptr(lab), *(_dptr(v) for v in out.values())))
        out["modules"] = np.unique(lab[lab > 0]).astype(np.int32)
        return out

    def hub_nodes(self, labels) -> dict:
        """Per module the node with the largest ``kWithin``, ties to the
        lowest node index: ``{label: node name}``."""
        lab = self._labels(labels)
        k = self.intramodular_connectivity(lab)
        hubs = {}
        for m in k["modules"]:
            idx = np.flatnonzero(lab == m)
            hubs[int(m)] = self.node_names[int(idx[int(np.argmax(k["kWithin"][idx]))])]
        return hubs

    def node_order(self, labels, orderModules: bool = True) -> dict:
        """NetRep's ``nodeOrder`` for this one dataset (R/orderNodes.R, mean =
        FALSE, every node present). Modules stand in the leaf order of the
        complete-linkage tree of their eigengenes on 1 - cor
        (netrep_EigengeneTree, netrep_HclustFinish: R's ``hclust`` default);
        with one module or ``orderModules=False`` in increasing label order.
        Within a module the nodes stand by decreasing ``kWithin``, ties in
        node order. ``nodes``: the node names flattened (simplify = TRUE);
        ``modules``: ``{label: [node names]}`` in module order."""
        lab = self._labels(labels)
        k = self.intramodular_connectivity(lab)
        mods = [int(m) for m in k["modules"]]
        if orderModules and len(mods) > 1:
            id_lo, id_hi, height = eigengeneTree(self.module_eigengenes(lab)["eigengenes"], "complete")
            _merge, _h, order, _r = hclustFinish(len(mods), id_lo, id_hi, height)
            mods = [mods[int(o) - 1] for o in order]
        by_module = {}
        for m in mods:
            idx = np.flatnonzero(lab == m)
            by_module[m] = [self.node_names[int(i)] for i in idx[np.argsort(-k["kWithin"][idx], kind="stable")]]
        return {"nodes": [nm for m in mods for nm in by_module[m]], "modules": by_module}

    def sample_order(self, labels) -> dict:
        """NetRep's ``sampleOrder`` (R/orderSamples.R): per module the
        0-based sample indices by decreasing eigengene value, ties in sample
        order: ``{label: indices}``, from ``module_eigengenes``."""
        e = self.module_eigengenes(labels)
        return {int(m): np.argsort(-e["eigengenes"][:, j], kind="stable") for j, m in enumerate(e["modules"])}


def _i32ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def eigengeneGroups(eigengenes, cutHeight: float):
    """The eigengene tree and its cut (netrep_EigengeneGroups; a pure host
    function): ``(group, heights)`` of an (S x M) eigengene matrix -- the
    0-based index of the first module of every module's group, and the M - 1
    average-linkage heights on 1 - cor in merge order."""
    e = np.asfortranarray(np.asarray(eigengenes, dtype=np.float64))
    if e.ndim != 2:
        raise L.NetRepError(L.NR_ERR_INVALID, "eigengenes must be a samples x modules matrix")
    s, m = e.shape
    group = np.zeros(max(m, 1), dtype=np.int32)
    heights = np.zeros(max(m - 1, 1))
    L.check_api(L.load().netrep_EigengeneGroups(_dptr(e), s, m, float(cutHeight), _i32ptr(group), _dptr(heights)))
    return group[:m], heights[:max(m - 1, 0)]


LINKAGES = {"average": 0, "complete": 1}


def eigengeneTree(eigengenes, linkage: str = "complete"):
    """The eigengene tree (netrep_EigengeneTree; a pure host function) of an
    (S x M) eigengene matrix on 1 - cor with ``linkage`` "average" or
    "complete": ``(id_lo, id_hi, height)``, M - 1 merges in discovery order
    as ``hclustFinish`` takes them."""
    e = np.asfortranarray(np.asarray(eigengenes, dtype=np.float64))
    if e.ndim != 2:
        raise L.NetRepError(L.NR_ERR_INVALID, "eigengenes must be a samples x modules matrix")
    if linkage not in LINKAGES:
        raise L.NetRepError(L.NR_ERR_INVALID, f"unknown linkage {linkage!r}: one of 'average', 'complete'")
    s, m = e.shape
    id_lo = np.zeros(max(m - 1, 1), dtype=np.int32)
    id_hi = np.zeros(max(m - 1, 1), dtype=np.int32)
    height = np.zeros(max(m - 1, 1))
    L.check_api(L.load().netrep_EigengeneTree(_dptr(e), s, m, LINKAGES[linkage], _i32ptr(id_lo), _i32ptr(id_hi),
                                              _dptr(height)))
    k = max(m - 1, 0)
    return id_lo[:k], id_hi[:k], height[:k]


def intramodularConnectivity(labels, kTotal, kMod) -> dict:
    """``kWithin``, ``kOut`` and ``kDiff`` from a module-connectivity table
    (netrep_IntramodularConnectivity; a pure host function): ``kMod`` (n x M,
    its columns the distinct positive labels in increasing order) and
    ``kTotal`` (n) as ``FromDataDataset.module_connectivity`` returns them."""
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    tot = np.ascontiguousarray(kTotal, dtype=np.float64)
    table = np.asfortranarray(np.asarray(kMod, dtype=np.float64))
    m = int(np.unique(lab[lab > 0]).size) if lab.ndim == 1 else 0
    if lab.ndim != 1 or tot.shape != lab.shape or table.shape != (lab.size, max(m, 1)):
        raise L.NetRepError(L.NR_ERR_INVALID, "labels and kTotal must be vectors of one length n, kMod n x modules")
    out = {k: np.zeros(max(lab.size, 1)) for k in ("kWithin", "kOut", "kDiff")}
    L.check_api(L.load().netrep_IntramodularConnectivity(lab.size, _i32ptr(lab), _dptr(tot), _dptr(table),
                                                         *(_dptr(v) for v in out.values())))
    return {k: v[:lab.size] for k, v in out.items()}


def mergeLabels(labels, moduleLabels, group, relabel: bool = False) -> np.ndarray:
    """One merge step (netrep_MergeLabels; a pure host function): nodes of
    ``moduleLabels[m]`` get ``moduleLabels[group[m]]``; with ``relabel`` the
    result is renumbered 1, 2, ... by decreasing size."""
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    mods = np.ascontiguousarray(moduleLabels, dtype=np.int32)
    grp = np.ascontiguousarray(group, dtype=np.int32)
    if lab.ndim != 1 or mods.shape != grp.shape or mods.ndim != 1:
        raise L.NetRepError(L.NR_ERR_INVALID, "labels, moduleLabels and group must be vectors, the last two alike")
    out = np.zeros(max(lab.size, 1), dtype=np.int32)
    L.check_api(L.load().netrep_MergeLabels(lab.size, _i32ptr(lab), mods.size, _i32ptr(mods), _i32ptr(grp),
                                            int(bool(relabel)), _i32ptr(out)))
    return out[:lab.size]


def trimModulesKME(labels, kME, minSize: int, minKMEtoStay: float = 0.3, minCoreKME: float = 0.5,
                   minCoreKMESize=None) -> np.ndarray:
    """The kME trimming on host arrays (netrep_TrimModulesKME; a pure host
    function): ``kME`` each node's correlation with its own module's
    eigengene. Rules as ``FromDataDataset.trim_modules``."""
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    own = np.ascontiguousarray(kME, dtype=np.float64)
    if lab.ndim != 1 or own.shape != lab.shape:
        raise L.NetRepError(L.NR_ERR_INVALID, "labels and kME must be vectors of one length")
    out = np.zeros(max(lab.size, 1), dtype=np.int32)
    core = -1 if minCoreKMESize is None else int(minCoreKMESize)
    L.check_api(L.load().netrep_TrimModulesKME(lab.size, _i32ptr(lab), _dptr(own), float(minKMEtoStay),
                                               float(minCoreKME), core, int(minSize), _i32ptr(out)))
    return out[:lab.size]


def hclustFinish(n: int, id_lo, id_hi, height):
    """Discovery-order merges (``Engine.hclust_average``) to R's hclust
    components (netrep_HclustFinish; a pure host function): ``(merge, height,
    order, n_repairs)``."""
    n = int(n)
    m = max(n - 1, 0)
    lo = np.ascontiguousarray(id_lo, dtype=np.int32)
    hi = np.ascontiguousarray(id_hi, dtype=np.int32)
    h_in = np.ascontiguousarray(height, dtype=np.float64)
    if lo.shape != (m,) or hi.shape != (m,) or h_in.shape != (m,):
        raise L.NetRepError(L.NR_ERR_INVALID, "id_lo, id_hi and height must hold n - 1 entries each")
    merge = np.zeros((m, 2), dtype=np.int32, order="F")
    h = np.zeros(m, dtype=np.float64)
    order = np.zeros(max(n, 1), dtype=np.int32)
    repairs = C.c_int32()
    L.check_api(L.load().netrep_HclustFinish(n, _i32ptr(lo), _i32ptr(hi), _dptr(h_in), _i32ptr(merge), _dptr(h),
                                             _i32ptr(order), C.byref(repairs)))
    return merge, h, order, int(repairs.value)


def cutreeStatic(tree: Mapping, cutHeight: float, minSize: int = 50) -> np.ndarray:
    """A static cut of an hclust tree (``FromDataDataset.hclust()``, or any
    mapping with ``merge`` and ``height``) into module labels, after WGCNA's
    cutreeStatic (netrep_CutreeStatic; a pure host function): every merge
    with height <= ``cutHeight`` is applied, clusters of fewer than
    ``minSize`` nodes get 0, the rest are numbered 1, 2, ... by decreasing
    size (ties: the cluster that appears first in node order)."""
    merge = np.asfortranarray(np.asarray(tree["merge"], dtype=np.int32))
    height = np.ascontiguousarray(tree["height"], dtype=np.float64)
    m = height.shape[0]
    if merge.shape != (m, 2):
        raise L.NetRepError(L.NR_ERR_INVALID, "merge must be (n - 1) x 2 and height n - 1 long")
    labels = np.zeros(m + 1, dtype=np.int32)
    L.check_api(L.load().netrep_CutreeStatic(m + 1, _i32ptr(merge), _dptr(height), float(cutHeight), int(minSize),
                                             _i32ptr(labels)))
    return labels


def DetectModulesFromData(data: RMatrix, beta: float, cutHeight: float, minSize: int = 50,
                          networkType: str = "unsigned", corType: str = "pearson", tom: bool = True,
                          scaleData: bool = True, mergeCutHeight: Optional[float] = None,
                          minKMEtoStay: Optional[float] = None, minCoreKME: float = 0.5,
                          minCoreKMESize: Optional[int] = None) -> dict:
    """Module labels from the data matrix alone: the network (the TOM unless
    ``tom=False``) is built on the GPU, its average-linkage dendrogram on
    1 - net is built there too, and a static cut at ``cutHeight`` with
    ``minSize`` gives the labels; no n x n matrix exists on the host. Returns
    ``{"moduleAssignments": {node name: label}, "tree": ...}``: labels as
    strings, the background "0", directly usable as ``moduleAssignments`` of
    modulePreservationFromData; ``tree`` as ``FromDataDataset.hclust()``.
    With ``minKMEtoStay`` and / or ``mergeCutHeight`` the cut is followed, on
    the same resident dataset, by the kME trimming
    (``FromDataDataset.trim_modules`` with ``minSize``, ``minCoreKME``,
    ``minCoreKMESize``) and then the merging of close modules
    (``merge_close_modules`` at ``mergeCutHeight``, relabelled by size), in
    that order; the result gains ``unmergedAssignments`` (the labels before
    the merge, as strings), ``eigengenes`` (S x M of the final modules) and
    ``rounds``. With both ``None`` nothing else runs."""
    with FromDataDataset(data, beta, networkType=networkType, scaleData=scaleData, tom=tom, corType=corType) as ds:
        tree = ds.hclust()
        labels = cutreeStatic(tree, cutHeight, minSize)
        if mergeCutHeight is None and minKMEtoStay is None:
            extra = {}
        else:
            if minKMEtoStay is not None and (labels > 0).any():
                labels = ds.trim_modules(labels, minSize, minKMEtoStay, minCoreKME, minCoreKMESize)
            unmerged = labels
            extra = {"unmergedAssignments": {nm: str(int(lab)) for nm, lab in zip(tree["labels"], unmerged)},
                     "eigengenes": np.zeros((ds.n_samples, 0), order="F"), "rounds": 0}
            if (labels > 0).any():
                if mergeCutHeight is not None:
                    merged = ds.merge_close_modules(labels, mergeCutHeight, relabel=True)
                    labels = merged["labels"]
                    extra.update(eigengenes=merged["eigengenes"], rounds=merged["rounds"])
                else:
                    extra.update(eigengenes=ds.module_eigengenes(labels)["eigengenes"])
    out = {"moduleAssignments": {nm: str(int(lab)) for nm, lab in zip(tree["labels"], labels)}, "tree": tree}
    out.update(extra)
    return out


def IntermediatePropertiesFromData(dData: RMatrix, beta: float, tNodeNames, moduleAssignments, modules,
                                   networkType: str = "unsigned", scaleData: bool = False, tom: bool = False,
                                   corType: str = "pearson") -> dict:
    """IntermediateProperties on a discovery dataset given as its data matrix
    alone (netrep_IntermediatePropertiesFromData): ``dData`` (scaled already
    unless ``scaleData``, as IntermediateProperties wants it) is the only
    upload; correlation and network are built on the GPU and never exist on
    the host."""
    d_names, x = _named_data(dData, "dData")
    s, n = x.shape
    call = _IntermediateCall(tNodeNames, moduleAssignments, modules, True)
    dn, _k1 = _strv(d_names)
    L.check_api(L.load().netrep_IntermediatePropertiesFromData(
        _dptr(x), int(bool(scaleData)), L.net_type_code(networkType, tom, corType), float(beta), s, n, dn,
        *call.args))
    return call.result()


def NetPropsFromData(data: RMatrix, beta: float, moduleAssignments, modules, networkType: str = "unsigned",
                     scaleData: bool = True, tom: bool = False, corType: str = "pearson") -> dict:
    """NetProps on a dataset given as its data matrix alone
    (netrep_NetPropsFromData): ``data`` is raw and scaled on the GPU (as
    NetProps scales) unless ``scaleData=False``; the network is built there."""
    node_names, x = _named_data(data, "data")
    s, n = x.shape
    call = _NetPropsCall(moduleAssignments, modules, s, True)
    nn, _k1 = _strv(node_names)
    L.check_api(L.load().netrep_NetPropsFromData(
        _dptr(x), int(bool(scaleData)), L.net_type_code(networkType, tom, corType), float(beta), s, n, nn,
        *call.args))
    return call.result()


def _as_name_list(x):
    return [str(x)] if isinstance(x, (str, bytes)) or not hasattr(x, "__iter__") else [str(v) for v in x]


def _per_pair(value, di, ti):
    """`value`, or value[di][ti] of a nested mapping."""
    if isinstance(value, Mapping):
        inner = value.get(di)
        return inner.get(ti) if isinstance(inner, Mapping) else inner
    return value


def modulePreservationFromData(datasets: Mapping, beta, moduleAssignments: Mapping, modules=None, discovery=None,
                               test=None, nPerm: int = 10000, nullHypothesis: str = "overlap",
                               alternative: str = "greater", seed: int = DEFAULT_SEED,
                               networkType: str = "unsigned", scaleData: bool = True, tom: bool = False,
                               corType: str = "pearson", pi=None) -> dict:
    """modulePreservation's loop over (discovery, test) pairs
    (R/modulePreservation.R:553-620) from data matrices alone: no n x n matrix
    exists on the host. ``datasets`` {name: RMatrix (samples x nodes, colnames
    the node names)}; ``beta`` a scalar or {name: beta}; ``moduleAssignments``
    {discovery name: {node: label}}; ``modules`` None (every label but the
    background "0", in orderAsNumeric order), a list, or {discovery: list};
    ``discovery`` a name or names (default: the first dataset); ``test`` a
    name or names, or {discovery: names} (default: every other dataset).
    One FromDataDataset per dataset name is built on first use and closed
    when the call returns or raises. ``pi``: explicit shuffles for every pair,
    or {discovery: {test: pi}}. Returns ``res[discovery][test]`` with
    modulePreservation's entries (observed, nulls, p.values, nVarsPresent,
    propVarsPresent, totalSize, alternative, contingency -- the matrix, its
    dimnames beside it, None without module assignments for the test dataset)
    plus ``modules``, the row names; a result combineAnalyses accepts."""
    from .contingency import contingencyTable, order_as_numeric, total_size
    from .pvalues import permutationTest

    names = [str(k) for k in datasets]
    data = {str(k): v for k, v in datasets.items()}
    assign = {str(k): v for k, v in moduleAssignments.items()}
    disc_names = [names[0]] if discovery is None else _as_name_list(discovery)
    pairs = []
    for di in disc_names:
        if test is None:
            tis = [t for t in names if t != di]
        elif isinstance(test, Mapping):
            tis = _as_name_list(test[di]) if di in test else []
        else:
            tis = _as_name_list(test)
        for ti in tis:
            if ti != di:                                 # R/modulePreservation.R:515-524
                pairs.append((di, ti))
    for nm in {x for p in pairs for x in p}:
        if nm not in data:
            raise L.NetRepError(L.NR_ERR_INVALID, f"no dataset named {nm!r}")
    for di in disc_names:
        if di not in assign:
            raise L.NetRepError(L.NR_ERR_INVALID, f"no moduleAssignments for discovery dataset {di!r}")

    def beta_of(nm):
        return float(beta[nm]) if isinstance(beta, Mapping) else float(beta)

    def modules_of(di):
        m = modules.get(di) if isinstance(modules, Mapping) else modules
        if m is None:
            _n, labels = _assignments(assign[di])
            return order_as_numeric([lab for lab in dict.fromkeys(labels) if lab != "0"])
        return order_as_numeric(_as_name_list(m))

    resident = {}

    def dataset(nm):
        if nm not in resident:
            resident[nm] = FromDataDataset(data[nm], beta_of(nm), networkType=networkType, scaleData=scaleData,
                                           tom=tom, corType=corType)
        return resident[nm]

    res = {}
    try:
        for di, ti in pairs:
            mods = modules_of(di)
            t_names = [str(n) for n in data[ti].colnames]
            ct = contingencyTable([assign[di], assign.get(ti)], mods, t_names)
            disc_props = dataset(di).intermediate_properties(t_names, assign[di], mods)
            perms = dataset(ti).permutation_procedure(disc_props, assign[di], mods, nPerm,
                                                      nullHypothesis=nullHypothesis, seed=seed,
                                                      pi=_per_pair(pi, di, ti))
            out = {"observed": perms["observed"], "nVarsPresent": ct["varsPres"],
                   "propVarsPresent": ct["propVarsPres"], "alternative": alternative, "modules": mods,
                   "contingency": None}                     # without the test dataset's assignments
            if ct["contingency"] is not None:
                out["contingency"], rows, cols = ct["contingency"]
                out["contingency_dimnames"] = (rows, cols)
            if nPerm > 0:
                out["nulls"] = perms["nulls"]
                out["totalSize"] = total_size(nullHypothesis, ct["overlapVars"], len(t_names))
                out["p.values"] = permutationTest(out["nulls"], out["observed"], ct["varsPres"], out["totalSize"],
                                                  alternative, modules=mods)
            res.setdefault(di, {})[ti] = out
    finally:
        for d in resident.values():
            d.close()
    return res
