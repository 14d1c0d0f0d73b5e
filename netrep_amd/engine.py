"""Python handle on one engine context (one GPU, one resident dataset).

Thin wrapper over the ``nr_*`` C ABI (include/netrep_gpu.h). Arrays follow R's
layout: an ``(nrow, ncol)`` matrix is passed column-major, and the nulls cube
comes back as a Fortran-ordered ``(modules, statistics, permutations)`` array,
exactly the memory layout of the reference's ``arma::cube``
(src/permutations.cpp:55, :304).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def _f64(a) -> np.ndarray:
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def _ptr(a, ctype=C.c_double):
    if a is None:
        return None
    return a.ctypes.data_as(C.POINTER(ctype))


# The 16 phase-stamp slots as include/netrep_gpu.h (nr_set_stamps) lists them.
STAMP_SLOTS = ["index", "gram", "lanczos_setup", "matvec", "three_term_omega", "statistics", "q_update",
               "ritz_checks", "start_column", "reorth", "ritz_vector", "node_contributions", "ritz_coefficients",
               "check_eigenvalue", "check_residual", "s15"]


class Engine:
    """One GPU context. ``device`` is the HIP ordinal."""

    # side of the from-data kernel's workgroup tile (kNetbuildTile, csrc/kernels.h)
    NETBUILD_TILE = 64
    # rows of a column the correlation-type kernels stage in LDS (kCorLdsRows,
    # csrc/kernels.h): longer columns are swept in global memory. Up to a
    # quarter of it (COR_WAVE_ROWS) a wave owns a column, four per workgroup.
    COR_LDS_ROWS = 2048
    COR_WAVE_ROWS = COR_LDS_ROWS // 4
    # candidate powers one soft_connectivity call takes (kSftMaxPowers, csrc/kernels.h)
    SFT_MAX_POWERS = 32

    def __init__(self, device: int = 0):
        self._lib = L.load()
        h = C.c_void_p()
        rc = self._lib.nr_ctx_create(int(device), C.byref(h))
        if rc != L.NR_OK:
            raise L.NetRepError(rc, self._lib.nr_last_error(None).decode())
        self._h = h
        self.device = device
        self.n_stat = None
        self.n_rows = 0
        self.n_null = 0

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.nr_ctx_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        L.check(rc, self._h)

    # -- dataset ----------------------------------------------------------
    def set_dataset(self, corr, net, data=None):
        """Host numpy matrices: corr, net (N x N) and optional scaled data (S x N)."""
        corr = _f64(corr)
        net = _f64(net)
        n = corr.shape[0]
        if corr.shape != (n, n) or net.shape != (n, n):
            raise ValueError("corr and net must be square and of equal size")
        d = None
        s = 0
        if data is not None:
            d = _f64(data)
            s = d.shape[0]
            if d.shape[1] != n:
                raise ValueError("data must have one column per node")
        self._check(self._lib.nr_set_dataset(self._h, _ptr(corr), _ptr(net), _ptr(d), n, s, L.NR_HOST))
        self.n_stat = 7 if data is not None else 4
        self.n_nodes = n
        self.n_samples = s

    def set_dataset_from_data(self, data, beta, net_type="unsigned", scale=True, tom=False, cor_type="pearson"):
        """The resident dataset from the data matrix alone (S x N, host numpy):
        only `data` is uploaded (scaled on the device unless ``scale=False``:
        already scaled); corr = cor(data) and net (``net_type`` 'unsigned'
        |corr|^beta, 'signed' ((1 + corr) / 2)^beta, 'signed_hybrid' corr^beta
        for corr > 0, else 0) are built in HBM (nr_set_dataset_from_data).
        ``tom=True``: the resident net is the topological overlap matrix of
        that adjacency (NR_NET_TOM: WGCNA's unsigned TOM, TOMDenom "min"),
        computed on the device too; corr is the same either way.
        ``cor_type`` 'spearman' (the correlation of the average ranks) or
        'bicor' (WGCNA's biweight midcorrelation with its defaults): corr is
        of that type, from a transient transform of the resident scaled
        block; the data block itself, and so the data statistics, stay the
        scaled data (include/netrep_gpu.h has the definitions)."""
        d = _f64(data)
        if d.ndim != 2:
            raise ValueError("data must be a samples x nodes matrix")
        s, n = d.shape
        self._check(self._lib.nr_set_dataset_from_data(self._h, _ptr(d), n, s, L.NR_HOST,
                                                       L.NR_SCALE_DATA if scale else 0,
                                                       L.net_type_code(net_type, tom, cor_type), float(beta)))
        self.n_stat = 7
        self.n_nodes = n
        self.n_samples = s

    def matrices(self):
        """(corr, net) of the resident dataset as host arrays (nr_get_dataset_matrices)."""
        n, _s = self.shape()
        corr = np.empty((n, n), dtype=np.float64, order="F")
        net = np.empty((n, n), dtype=np.float64, order="F")
        self._check(self._lib.nr_get_dataset_matrices(self._h, _ptr(corr), _ptr(net)))
        return corr, net

    def netbuild_ms(self) -> float:
        """Device time in ms of the from-data build of the resident matrices
        (nr_netbuild_ms), 0 for a dataset made any other way. A copy reports
        the figure of the dataset it was copied from."""
        ms = C.c_double()
        self._check(self._lib.nr_netbuild_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def tom_ms(self) -> float:
        """Device time in ms of the topological-overlap step of a from-data
        build with ``tom=True`` (nr_tom_ms: extract, degrees and the TOM
        kernel; not part of netbuild_ms), 0 for any other dataset. A copy
        reports its source's figure."""
        ms = C.c_double()
        self._check(self._lib.nr_tom_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def cor_ms(self) -> float:
        """Device time in ms of the correlation-type transform of a from-data
        build with ``cor_type`` 'spearman' or 'bicor' (nr_cor_ms; not part of
        netbuild_ms or tom_ms), 0 for Pearson or any other dataset. A copy
        reports its source's figure."""
        ms = C.c_double()
        self._check(self._lib.nr_cor_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def soft_connectivity(self, data, powers, net_type="unsigned", scale=True, cor_type="pearson"):
        """The soft-threshold connectivities of WGCNA's pickSoftThreshold from
        the data matrix alone (S x N, host numpy; nr_soft_connectivity): an
        ``(N, len(powers))`` Fortran-ordered array, column m holding
        ``k_i = sum_{u != i} b_iu ** powers[m]`` with b the base of
        ``net_type`` (|cor|, (1 + cor) / 2, or cor where cor > 0 else 0) and
        cor of ``cor_type``. No N x N matrix exists on the host or the device,
        and the engine's resident dataset and modules are not touched. A
        constant column makes every connectivity NaN (no error here;
        ``PickSoftThreshold`` raises). At most ``SFT_MAX_POWERS`` powers,
        finite and > 0; order and duplicates are kept."""
        d = _f64(data)
        if d.ndim != 2:
            raise ValueError("data must be a samples x nodes matrix")
        s, n = d.shape
        p = np.ascontiguousarray(np.atleast_1d(powers), dtype=np.float64)
        if p.ndim != 1:
            raise ValueError("powers must be a vector")
        k = np.empty((n, p.size), dtype=np.float64, order="F")
        self._check(self._lib.nr_soft_connectivity(self._h, _ptr(d), n, s, int(bool(scale)),
                                                   L.net_type_code(net_type, False, cor_type), _ptr(p),
                                                   int(p.size), _ptr(k)))
        return k

    def sft_ms(self) -> float:
        """Device time in ms of the two kernels of this engine's last
        ``soft_connectivity`` call (nr_sft_ms), 0 before the first."""
        ms = C.c_double()
        self._check(self._lib.nr_sft_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def set_sft_row_groups(self, row_groups: int):
        """Test knob (nr_set_sft_row_groups): the row-group count of later
        ``soft_connectivity`` calls; 0 restores the default."""
        self._check(self._lib.nr_set_sft_row_groups(self._h, int(row_groups)))

    def hclust_average(self):
        """The average-linkage dendrogram of the resident dataset's nodes on
        d = 1 - net (nr_hclust_average; include/netrep_gpu.h has the rules),
        raw: ``(id_lo, id_hi, height, size)`` of the n - 1 merges in discovery
        order, ids 0 .. n-1 nodes and n + t the cluster of step t. The
        resident dataset is not changed."""
        n, _s = self.shape()
        m = max(n - 1, 0)
        id_lo = np.zeros(m, dtype=np.int32)
        id_hi = np.zeros(m, dtype=np.int32)
        height = np.zeros(m, dtype=np.float64)
        size = np.zeros(m, dtype=np.float64)
        self._check(self._lib.nr_hclust_average(self._h, id_lo.ctypes.data_as(L._i32p), id_hi.ctypes.data_as(L._i32p),
                                                _ptr(height), _ptr(size)))
        return id_lo, id_hi, height, size

    def hclust_ms(self) -> float:
        """Device time in ms of the extract and all chain launches of this
        engine's last ``hclust_average`` call (nr_hclust_ms)."""
        ms = C.c_double()
        self._check(self._lib.nr_hclust_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def hclust_info(self) -> dict:
        """Of the last ``hclust_average`` call (nr_hclust_info): nearest-
        neighbour ``searches``, chain ``launches``, device ``scratch_bytes``."""
        s, l, b = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.nr_hclust_info(self._h, C.byref(s), C.byref(l), C.byref(b)))
        return {"searches": int(s.value), "launches": int(l.value), "scratch_bytes": int(b.value)}

    def set_hclust_merges_per_launch(self, merges: int):
        """Test knob (nr_set_hclust_merges_per_launch): merges per chain
        launch of later ``hclust_average`` calls; 0 restores the default."""
        self._check(self._lib.nr_set_hclust_merges_per_launch(self._h, int(merges)))

    def set_dataset_files(self, corr_path, net_path, data_path=None, objects=(None, None, None),
                          scale_data=True):
        """disk.matrix files (saveRDS output, or objects of a save() archive)
        straight to HBM; `data` is scaled on the device. Returns the node names
        (the network file's column names)."""
        enc = lambda x: None if x is None else str(x).encode()  # noqa: E731
        self._check(self._lib.nr_set_dataset_files(self._h, enc(corr_path), enc(net_path), enc(data_path),
                                                   enc(objects[0]), enc(objects[1]), enc(objects[2]),
                                                   int(bool(scale_data))))
        self.n_stat = 7 if data_path is not None else 4
        self.n_nodes, self.n_samples = self.shape()
        return self.colnames()

    def colnames(self):
        """Column names of the resident dataset (nr_dataset_colnames): those of
        the files it was loaded from, carried by its copies; [] otherwise."""
        need = C.c_int64()
        self._check(self._lib.nr_dataset_colnames(self._h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(max(need.value, 1))
        self._check(self._lib.nr_dataset_colnames(self._h, buf, need.value, C.byref(need)))
        names = buf.raw[:need.value].split(b"\0")[:-1] if need.value else []
        return [x.decode() for x in names]

    def set_dataset_device(self, corr_ptr: int, net_ptr: int, data_ptr, n_nodes: int, n_samples: int):
        """Device pointers (e.g. torch tensors after an RCCL broadcast). The
        engine reads them on its own stream: the producer's work must be
        complete (e.g. torch.cuda.synchronize()) -- torch's streams belong to
        its own HIP runtime and are not ordered with the engine's."""
        self._check(self._lib.nr_set_dataset(self._h, C.cast(corr_ptr, L._dp), C.cast(net_ptr, L._dp),
                                             C.cast(data_ptr, L._dp) if data_ptr else None,
                                             n_nodes, n_samples, L.NR_DEVICE))
        self.n_stat = 7 if data_ptr else 4
        self.n_nodes = n_nodes
        self.n_samples = n_samples if data_ptr else 0

    def broadcast_dataset_to(self, others):
        """This context's resident dataset to every context in `others`
        (nr_broadcast_dataset: scatter + all-gather of peer copies)."""
        hs = (C.c_void_p * (1 + len(others)))(self._h.value, *[o._h.value for o in others])
        self._check(self._lib.nr_broadcast_dataset(hs, 1 + len(others)))
        for o in others:
            o.n_stat, o.n_nodes, o.n_samples = self.n_stat, self.n_nodes, self.n_samples

    def set_host_threads(self, n: int):
        """Host threads of this context's staging copies (nr_ctx_set_host_threads)."""
        self._check(self._lib.nr_ctx_set_host_threads(self._h, int(n)))

    def copy_dataset_from(self, other: "Engine"):
        """Device-to-device copy of another context's resident dataset
        (nr_copy_dataset: over xGMI between GPUs)."""
        self._check(self._lib.nr_copy_dataset(self._h, other._h))
        self.n_stat = other.n_stat
        self.n_nodes = other.n_nodes
        self.n_samples = other.n_samples

    def shape(self):
        """(n_nodes, n_samples) of the resident dataset; (0, 0) when there is none."""
        n, s_ = C.c_int64(), C.c_int64()
        self._check(self._lib.nr_dataset_shape(self._h, C.byref(n), C.byref(s_)))
        return n.value, s_.value

    def symmetric(self) -> bool:
        v = C.c_int()
        self._check(self._lib.nr_dataset_symmetric(self._h, C.byref(v)))
        return bool(v.value)

    def finite(self):
        """(corr all finite, net all finite) of the resident dataset -- CheckFinite
        (src/checkFinite.cpp:21-28) fused into the upload's symmetry pass."""
        c, n = C.c_int(), C.c_int()
        self._check(self._lib.nr_dataset_finite(self._h, C.byref(c), C.byref(n)))
        return bool(c.value), bool(n.value)

    # -- modules ----------------------------------------------------------
    def set_modules(self, n_rows, row_of, node_off, test_idx, null_pos, disc_corr, disc_degree,
                    disc_contrib=None):
        row_of = np.ascontiguousarray(row_of, dtype=np.int32)
        node_off = np.ascontiguousarray(node_off, dtype=np.int64)
        test_idx = np.ascontiguousarray(test_idx, dtype=np.int32)
        null_pos = None if null_pos is None else np.ascontiguousarray(null_pos, dtype=np.int32)
        disc_corr = np.ascontiguousarray(disc_corr, dtype=np.float64)
        disc_degree = np.ascontiguousarray(disc_degree, dtype=np.float64)
        disc_contrib = None if disc_contrib is None else np.ascontiguousarray(disc_contrib, dtype=np.float64)
        self._keep = (row_of, node_off, test_idx, null_pos, disc_corr, disc_degree, disc_contrib)
        self._check(self._lib.nr_set_modules(
            self._h, int(n_rows), int(row_of.size), _ptr(row_of, C.c_int32), _ptr(node_off, C.c_int64),
            _ptr(test_idx, C.c_int32), _ptr(null_pos, C.c_int32), _ptr(disc_corr), _ptr(disc_degree),
            _ptr(disc_contrib)))
        self.n_rows = int(n_rows)
        self.node_off = node_off

    def set_null_pool(self, null_idx):
        null_idx = np.ascontiguousarray(null_idx, dtype=np.int32)
        self._check(self._lib.nr_set_null_pool(self._h, _ptr(null_idx, C.c_int32), int(null_idx.size)))
        self.n_null = int(null_idx.size)

    # -- statistics -------------------------------------------------------
    def observed(self) -> np.ndarray:
        out = np.empty((self.n_rows, self.n_stat), dtype=np.float64, order="F")
        self._check(self._lib.nr_observed(self._h, _ptr(out)))
        return out

    def gram_table(self) -> bool:
        """Whether the resident dataset carries the Gram table (nr_gram_table)."""
        on = C.c_int()
        self._check(self._lib.nr_gram_table(self._h, C.byref(on)))
        return bool(on.value)

    def gram_table_ms(self) -> float:
        """Build time of the resident Gram table in ms (nr_gram_table_ms), 0 without one."""
        ms = C.c_double()
        self._check(self._lib.nr_gram_table_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def observed_async(self):
        """Enqueue the observed statistics on the context's second stream
        (nr_observed_async); collect them with observed_wait()."""
        self._check(self._lib.nr_observed_async(self._h))

    def observed_wait(self) -> np.ndarray:
        out = np.empty((self.n_rows, self.n_stat), dtype=np.float64, order="F")
        self._check(self._lib.nr_observed_wait(self._h, _ptr(out)))
        return out

    def run(self, perm_begin: int, perm_end: int, seed: int = 0, pi=None) -> np.ndarray:
        n = perm_end - perm_begin
        out = np.empty((self.n_rows, self.n_stat, n), dtype=np.float64, order="F")
        pi_arr = None
        if pi is not None:
            pi_arr = np.ascontiguousarray(pi, dtype=np.uint32)
            if pi_arr.shape != (n, self.n_null):
                raise ValueError(f"pi must have shape ({n}, {self.n_null})")
        self._check(self._lib.nr_run(self._h, int(perm_begin), int(perm_end), int(seed) & (2**64 - 1),
                                     _ptr(pi_arr, C.c_uint32), _ptr(out)))
        return out

    def run_device(self, perm_begin: int, perm_end: int, seed: int, out_ptr: int, pi_ptr: int = 0):
        self._check(self._lib.nr_run_device(self._h, int(perm_begin), int(perm_end),
                                            int(seed) & (2**64 - 1), C.c_void_p(pi_ptr or None),
                                            C.c_void_p(out_ptr)))

    def export_indices(self, perm_begin: int, perm_end: int, seed: int) -> np.ndarray:
        nodes = int(self.node_off[-1])
        out = np.empty((perm_end - perm_begin, nodes), dtype=np.int32)
        self._check(self._lib.nr_export_indices(self._h, int(perm_begin), int(perm_end),
                                                int(seed) & (2**64 - 1), _ptr(out, C.c_int32)))
        return out

    def module_vectors(self, node_off, idx, with_data: bool):
        """Per-module vectors on explicit index sets (CSR). Returns a dict of arrays."""
        node_off = np.ascontiguousarray(node_off, dtype=np.int64)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        n_mod = node_off.size - 1
        k = np.diff(node_off)
        cv = np.empty(max(int((k * (k - 1) // 2).sum()), 1))
        wd = np.empty(int(node_off[-1]))
        aw = np.empty(n_mod)
        nc = sp = coh = None
        if with_data:
            nc = np.empty(int(node_off[-1]))
            sp = np.empty(n_mod * self.n_samples)
            coh = np.empty(n_mod)
        self._check(self._lib.nr_module_vectors(self._h, int(n_mod), _ptr(node_off, C.c_int64),
                                                _ptr(idx, C.c_int32), _ptr(cv), _ptr(wd), _ptr(aw),
                                                _ptr(nc), _ptr(sp), _ptr(coh)))
        out = {"corr": cv[: int((k * (k - 1) // 2).sum())], "degree": wd, "avg_weight": aw}
        if with_data:
            out.update(contribution=nc, summary=sp.reshape(n_mod, self.n_samples), coherence=coh)
        return out

    def module_eigengenes(self, node_off, idx):
        """The eigengenes of explicit index sets (CSR) on the resident data
        (nr_module_eigengenes: the summary-profile kernels alone): a dict of
        ``eigengenes`` (S x M, Fortran order), ``varExplained`` (M) and
        ``kME`` (each node's correlation with its own module's eigengene, CSR
        order). The eigengenes also stay on the device for
        ``module_membership()``."""
        node_off = np.ascontiguousarray(node_off, dtype=np.int64)
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        n_mod = node_off.size - 1
        eig = np.empty((self.n_samples, max(n_mod, 0)), dtype=np.float64, order="F")
        ve = np.empty(max(n_mod, 0))
        nc = np.empty(int(node_off[-1]))
        self._check(self._lib.nr_module_eigengenes(self._h, int(n_mod), _ptr(node_off, C.c_int64),
                                                   _ptr(idx, C.c_int32), _ptr(eig), _ptr(ve), _ptr(nc)))
        return {"eigengenes": eig, "varExplained": ve, "kME": nc}

    def module_membership(self, n_mod: int, eigengenes=None) -> np.ndarray:
        """kME of every node of the resident data with ``n_mod`` eigengenes
        (nr_module_membership): an ``(n_nodes, n_mod)`` Fortran-ordered array.
        ``eigengenes`` None: those of the last ``module_eigengenes`` call,
        still on the device; else an ``(S, n_mod)`` host array, uploaded."""
        e = None
        if eigengenes is not None:
            e = _f64(eigengenes)
            if e.shape != (self.n_samples, int(n_mod)):
                raise ValueError("eigengenes must be an (n_samples, n_mod) matrix")
        n, _s = self.shape()
        kme = np.empty((n, int(n_mod)), dtype=np.float64, order="F")
        self._check(self._lib.nr_module_membership(self._h, int(n_mod), _ptr(e), _ptr(kme)))
        return kme

    def membership_ms(self) -> float:
        """Device time in ms of the two kernels of this engine's last
        ``module_membership`` call (nr_membership_ms)."""
        ms = C.c_double()
        self._check(self._lib.nr_membership_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def module_connectivity(self, n_mod: int, slot):
        """Connectivity of every node of the resident network to each of
        ``n_mod`` modules and to everything (nr_module_connectivity; the
        summation order is stated there). ``slot``: one module index
        0 .. n_mod - 1 per node, -1 unassigned. Returns ``(k_mod, k_total)``:
        an ``(n_nodes, n_mod)`` Fortran-ordered array and a vector."""
        n, _s = self.shape()
        sl = np.ascontiguousarray(slot, dtype=np.int32)
        if sl.shape != (n,):
            raise ValueError("slot must hold one module index per node")
        k_mod = np.empty((n, max(int(n_mod), 0)), dtype=np.float64, order="F")
        k_total = np.empty(n)
        self._check(self._lib.nr_module_connectivity(self._h, int(n_mod), _ptr(sl, C.c_int32), _ptr(k_total),
                                                     _ptr(k_mod)))
        return k_mod, k_total

    def connectivity_ms(self) -> float:
        """Device time in ms of the kernels of this engine's last
        ``module_connectivity`` call (nr_connectivity_ms)."""
        ms = C.c_double()
        self._check(self._lib.nr_connectivity_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def set_connectivity_module_tile(self, tile: int):
        """Test knob (nr_set_connectivity_module_tile): modules per pass of
        later ``module_connectivity`` calls, 0 the default."""
        self._check(self._lib.nr_set_connectivity_module_tile(self._h, int(tile)))

    def release_scratch(self):
        """Free the per-batch work buffers (nr_release_scratch)."""
        self._check(self._lib.nr_release_scratch(self._h))

    def scratch_bytes(self) -> int:
        """Device bytes of per-batch work buffers held (nr_scratch_bytes)."""
        b = C.c_int64()
        self._check(self._lib.nr_scratch_bytes(self._h, C.byref(b)))
        return int(b.value)

    def scale(self, data) -> np.ndarray:
        data = _f64(data)
        out = np.empty_like(data, order="F")
        self._check(self._lib.nr_scale(self._h, _ptr(data), data.shape[0], data.shape[1], _ptr(out)))
        return out

    # -- control / measurement -------------------------------------------
    def progress(self):
        d, t = C.c_int64(), C.c_int64()
        self._check(self._lib.nr_progress(self._h, C.byref(d), C.byref(t)))
        return d.value, t.value

    def cancel(self):
        self._check(self._lib.nr_cancel(self._h))

    def set_batch(self, perms_per_launch: int):
        self._check(self._lib.nr_set_batch(self._h, int(perms_per_launch)))

    def set_timing(self, enable: bool):
        self._check(self._lib.nr_set_timing(self._h, int(bool(enable))))

    def timing(self, kernel: int):
        ms, launches, items = C.c_double(), C.c_int64(), C.c_int64()
        self._check(self._lib.nr_get_timing(self._h, int(kernel), C.byref(ms), C.byref(launches),
                                            C.byref(items)))
        return ms.value, launches.value, items.value

    def diagnostics(self):
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.nr_get_diagnostics(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"eig_items": a.value, "eig_steps": b.value, "eig_cap_hits": c.value, "eig_reorths": d.value}

    def set_stamps(self, enable: bool):
        self._check(self._lib.nr_set_stamps(self._h, int(bool(enable))))

    def stamps(self):
        out = (C.c_uint64 * 16)()
        self._check(self._lib.nr_get_stamps(self._h, out))
        names = STAMP_SLOTS
        return dict(zip(names, list(out)))

    def reset_timing(self):
        self._check(self._lib.nr_reset_timing(self._h))

    def synchronize(self):
        self._check(self._lib.nr_synchronize(self._h))


def device_count() -> int:
    lib = L.load()
    n = C.c_int()
    lib.nr_device_count(C.byref(n))
    return n.value


def prp_table(seed: int, perm_begin: int, perm_end: int, n_null: int) -> np.ndarray:
    """Host evaluation of the keyed null-pool permutation (no GPU needed)."""
    lib = L.load()
    out = np.empty((perm_end - perm_begin, n_null), dtype=np.uint32)
    L.check(lib.nr_prp_table(int(seed) & (2**64 - 1), int(perm_begin), int(perm_end), int(n_null),
                             _ptr(out, C.c_uint32)))
    return out
