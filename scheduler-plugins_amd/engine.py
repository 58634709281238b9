"""ctypes wrapper over the spx_* C ABI (include/spx.h).  One Engine == one spx_engine == one
scheduler profile on one GPU.  Every method is a direct call into libspx.so; errors raise."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np

from ._abi import Table

PLUGINS = {
    "NodeResourcesAllocatable": 0,
    "TargetLoadPacking": 1,
    "LoadVariationRiskBalancing": 2,
    "NodeResourceTopologyMatch": 3,
    "NetworkOverhead": 4,
    "CapacityScheduling": 5,
    "TopologicalSort": 6,
}
ALLOCATABLE, TLP, LVRB, NRT, NETOVERHEAD, CAPACITY, TOPOSORT, LROC, PEAKS, SYSCHED = range(10)
NUM_PLUGINS = 13  # SPX_NUM_PLUGINS
COSCHED = 10  # SPX_PLUGIN_COSCHED: a PreFilter gate without tables; its entry of the weight vector is ignored
NODEMETA, PODSTATE = 11, 12  # SPX_PLUGIN_NODEMETA, SPX_PLUGIN_PODSTATE
NODEMETA_TYPE = {"Number": 0, "Timestamp": 1}  # SPX_NODEMETA_NUMBER / _TIMESTAMP
NODEMETA_STRATEGY = {"Highest": 0, "Lowest": 1, "Newest": 2, "Oldest": 3}  # SPX_NODEMETA_HIGHEST ...
INVALID_SCORE = -(1 << 63)  # NodeMetadata's invalidScore (math.MinInt64)
COSCHED_ST = {"BACKED_OFF": 1, "FEW_SIBLINGS": 2, "GATED": 3, "RESOURCE_GAP": 4}  # SPX_COSCHED_ST_*
PREEMPT_ST = {"CANDIDATE": 0, "NO_VICTIMS": 1, "NOT_FIT": 2, "QUOTA": 3, "ALL_REPRIEVED": 4, "REMOVE_TWICE": 5, "SKIPPED": 6}  # SPX_PREEMPT_ST_*


def mask_of(*plugins: int) -> int:
    m = 0
    for p in plugins:
        m |= 1 << p
    return m


class NrtPods(dict):
    """the dense NRT pod columns (spx_nrt_pods_soa, one entry per column) with `.long`: the containers of the batch's long rows — pods with
    more than SPX_NRT_MAX_CTRS containers, n_ctr == SPX_NRT_CTRS_LONG — as spx_flatten_nrt_long_pods returns them (dict: n_long,
    pod_row, ctr_ptr, ctr_kind, ctr_present, ctr_req)"""
    long: Optional[dict] = None


def long_rows_slice(lt: Optional[dict], rows, R: int) -> Optional[dict]:
    """the long-row table of batch rows [rows[0], rows[1]) with pod_row rebased to the slice (rows None: lt itself)"""
    if lt is None or rows is None:
        return lt
    b, e = rows
    pr = lt["pod_row"]
    k0, k1 = int(np.searchsorted(pr, b)), int(np.searchsorted(pr, e))
    ptr = lt["ctr_ptr"]
    c0, c1 = int(ptr[k0]), int(ptr[k1])
    return dict(n_long=k1 - k0, pod_row=(pr[k0:k1] - b).astype(np.int32), ctr_ptr=(ptr[k0:k1 + 1] - c0).astype(np.int32),
                ctr_kind=lt["ctr_kind"][c0:c1].copy(), ctr_present=lt["ctr_present"][c0:c1].copy(),
                ctr_req=lt["ctr_req"][c0 * max(R, 1):c1 * max(R, 1)].copy())


WIDE_POD_COLS = ("qos", "non_native", "req_ptr", "req_slot", "req_qty", "ctr_ptr", "ctr_kind", "ent_ptr", "ent_slot", "ent_qty")


def wide_rows_slice(pw: dict, rows) -> dict:
    """the wide NRT pod table (spx_nrt_pods_wide columns) of batch rows [rows[0], rows[1]), its offsets rebased (rows None: pw itself)"""
    if rows is None:
        return pw
    b, e = rows
    rp, cp, ep = pw["req_ptr"], pw["ctr_ptr"], pw["ent_ptr"]
    r0, r1, c0, c1 = int(rp[b]), int(rp[e]), int(cp[b]), int(cp[e])
    e0, e1 = int(ep[c0]), int(ep[c1])
    return dict(qos=pw["qos"][b:e].copy(), non_native=pw["non_native"][b:e].copy(),
                req_ptr=(rp[b:e + 1] - r0).astype(np.int32), req_slot=pw["req_slot"][r0:r1].copy(), req_qty=pw["req_qty"][r0:r1].copy(),
                ctr_ptr=(cp[b:e + 1] - c0).astype(np.int32), ctr_kind=pw["ctr_kind"][c0:c1].copy(),
                ent_ptr=(ep[c0:c1 + 1] - e0).astype(np.int32), ent_slot=pw["ent_slot"][e0:e1].copy(), ent_qty=pw["ent_qty"][e0:e1].copy())


def _rows(cols: Dict[str, np.ndarray], n_total: int, rows) -> Dict[str, np.ndarray]:
    """slice of per-pod SoA columns: every column holds a fixed number of entries per pod, pod-major"""
    if rows is None:
        return cols
    b, e = rows
    out = {}
    for k, v in cols.items():
        per = len(v) // max(n_total, 1)
        out[k] = np.ascontiguousarray(v[b * per:e * per]) if e > b else np.zeros(max(per, 1), v.dtype)
    return out


class Engine:
    def __init__(self, device: int = 0, _handle=None):
        from . import SpxError, header, lib

        self._lib = lib()
        self._hdr = header()
        self._err = SpxError
        self._owned = _handle is None
        if _handle is not None:  # an engine owned by a spx_multi (MultiEngine)
            self._h = _handle
        else:
            self._h = C.POINTER(self._hdr.opaque["spx_engine"])()
            rc = self._lib.spx_create(device, C.byref(self._h))
            if rc != 0:
                msg = self._lib.spx_last_error(None)
                raise SpxError(rc, msg.decode() if msg else "")
        self.n_nodes = 0
        self.n_pods = 0
        self.alloc_params: Optional[Table] = None
        self.tlp_params = Table(self._hdr, "spx_tlp_params", target_utilization=40, default_requests_milli=1000,
                                requests_multiplier=1.5)
        self.lvrb_params = Table(self._hdr, "spx_lvrb_params", safe_variance_margin=1.0, safe_variance_sensitivity=1.0)
        self.set_allocatable()

    # ------------------------------------------------------------------ plumbing
    def _ck(self, rc: int) -> None:
        if rc != 0:
            msg = self._lib.spx_last_error(self._h)
            raise self._err(rc, msg.decode() if msg else "")

    def close(self) -> None:
        if self._h:
            if self._owned:
                self._lib.spx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ------------------------------------------------------------------ options (per engine, spx_set_option)
    def set_option(self, option, value: int) -> None:
        """option: an SPX_OPT_* id or its name without the prefix, e.g. "REFERENCE_KERNELS"."""
        if isinstance(option, str):
            option = self._hdr.consts["SPX_OPT_" + option]
        self._ck(self._lib.spx_set_option(self._h, option, int(value)))

    def get_option(self, option) -> int:
        if isinstance(option, str):
            option = self._hdr.consts["SPX_OPT_" + option]
        v = C.c_int64()
        self._ck(self._lib.spx_get_option(self._h, option, C.byref(v)))
        return int(v.value)

    def nrt_pod_classes(self):
        """(representative rows, copied rows) of the uploaded NRT pod batch (spx_nrt_pod_classes); (n_pods, 0) when no two pods agree"""
        u, d = C.c_int64(), C.c_int64()
        self._ck(self._lib.spx_nrt_pod_classes(self._h, C.byref(u), C.byref(d)))
        return int(u.value), int(d.value)

    def peaks_pod_classes(self):
        """(rows that are the first with their cpu request, rows that repeat one) of the uploaded Peaks pod batch (spx_peaks_pod_classes)"""
        u, d = C.c_int64(), C.c_int64()
        self._ck(self._lib.spx_peaks_pod_classes(self._h, C.byref(u), C.byref(d)))
        return int(u.value), int(d.value)

    def tlp_pod_classes(self):
        """(rows evaluated, rows copied) of the uploaded trimaran pod batch in TargetLoadPacking's class form (spx_tlp_pod_classes)"""
        u, d = C.c_int64(), C.c_int64()
        self._ck(self._lib.spx_tlp_pod_classes(self._h, C.byref(u), C.byref(d)))
        return int(u.value), int(d.value)

    def tlp_order(self):
        """the pod row at every position of the class form's order (spx_tlp_fetch_order)"""
        rows = np.zeros(self.n_pods, np.int32)
        self._ck(self._lib.spx_tlp_fetch_order(self._h, rows.ctypes.data_as(C.POINTER(C.c_int32))))
        return rows

    def tlp_form(self) -> int:
        """what the last eval launched for TargetLoadPacking: 1 = every row in row order, 2 = the class form, 0 = neither (spx_tlp_form)"""
        return int(self._lib.spx_tlp_form(self._h))

    def sysched_pod_classes(self):
        """(pods that are the first of the batch with their syscall set, pods that repeat one) of the uploaded SySched pod batch
        (spx_sysched_pod_classes)"""
        u, d = C.c_int64(), C.c_int64()
        self._ck(self._lib.spx_sysched_pod_classes(self._h, C.byref(u), C.byref(d)))
        return int(u.value), int(d.value)

    def force_reference_kernels(self, *plugins: int) -> None:
        """run the reference-arithmetic sweep for these plugins (differential tests); no argument = back to the fast forms"""
        self.set_option("REFERENCE_KERNELS", mask_of(*plugins))

    def stats(self, reset: bool = False) -> np.ndarray:
        """cells re-evaluated by the exact float64 fallback of the fast sweeps, per plugin id (spx_fetch_stats)"""
        out = np.zeros(NUM_PLUGINS, np.int64)
        self._ck(self._lib.spx_fetch_stats(self._h, out.ctypes.data_as(C.POINTER(C.c_int64)), 1 if reset else 0))
        return out

    # ------------------------------------------------------------------ params
    def set_allocatable(self, mode: str = "Least", resources: Optional[Dict[int, int]] = None) -> None:
        """resources: {resource id: weight}; default = {memory: 1, cpu: 1<<20} (resource_allocation.go:36)."""
        if resources is None:
            resources = {1: 1, 0: 1 << 20}
        self.alloc_params = Table(self._hdr, "spx_allocatable_params", mode={"Least": 0, "Most": 1}[mode],
                                  n_res=len(resources), res=np.array(list(resources.keys()), dtype=np.int32),
                                  weight=np.array(list(resources.values()), dtype=np.int64))
        self._ck(self._lib.spx_set_allocatable_params(self._h, self.alloc_params.ref()))

    def set_tlp(self, target_utilization: int = 40, default_requests_milli: int = 1000, requests_multiplier: float = 1.5):
        self.tlp_params = Table(self._hdr, "spx_tlp_params", target_utilization=target_utilization,
                                default_requests_milli=default_requests_milli, requests_multiplier=requests_multiplier)
        self._ck(self._lib.spx_set_tlp_params(self._h, self.tlp_params.ref()))

    def set_lvrb(self, margin: float = 1.0, sensitivity: float = 1.0):
        self.lvrb_params = Table(self._hdr, "spx_lvrb_params", safe_variance_margin=margin,
                                 safe_variance_sensitivity=sensitivity)
        self._ck(self._lib.spx_set_lvrb_params(self._h, self.lvrb_params.ref()))

    def set_lroc(self, smoothing_window_size: int = 5, w_cpu: float = 0.5, w_mem: float = 0.5):
        self.lroc_params = Table(self._hdr, "spx_lroc_params", smoothing_window_size=smoothing_window_size,
                                 risk_limit_weight_cpu=w_cpu, risk_limit_weight_mem=w_mem)
        self._ck(self._lib.spx_set_lroc_params(self._h, self.lroc_params.ref()))

    # ------------------------------------------------------------------ flatten (host C++) + upload
    def flatten_alloc_nodes(self, nodes: Table, rc: Optional[Table]) -> np.ndarray:
        n = nodes.struct.n_nodes
        r = self.alloc_params.struct.n_res
        out = np.zeros((r, n), dtype=np.int64)
        self._ck(self._lib.spx_flatten_alloc_nodes(nodes.ref(), rc.ref() if rc else None, self.alloc_params.ref(),
                                                    out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def flatten_trimaran_nodes(self, nodes: Table, metrics: Table, assigned: Optional[Table]) -> Dict[str, np.ndarray]:
        n = nodes.struct.n_nodes
        cols = {
            "cap_cpu_milli": np.zeros(n, np.int64), "tlp_cpu_util": np.zeros(n, np.float64),
            "tlp_missing_milli": np.zeros(n, np.int64), "tlp_valid": np.zeros(n, np.uint8),
            "lv_alloc_cpu_milli": np.zeros(n, np.int64), "lv_alloc_mem": np.zeros(n, np.int64),
            "lv_cpu_avg": np.zeros(n, np.float64), "lv_cpu_std": np.zeros(n, np.float64),
            "lv_mem_avg": np.zeros(n, np.float64), "lv_mem_std": np.zeros(n, np.float64),
            "lv_flags": np.zeros(n, np.uint8),
        }
        fn = self._lib.spx_flatten_trimaran_nodes
        ptrs = [v.ctypes.data_as(t) for v, t in zip(cols.values(), fn.argtypes[4:])]
        self._ck(fn(nodes.ref(), metrics.ref(), assigned.ref() if assigned else None, self.tlp_params.ref(), *ptrs))
        return cols

    def flatten_trimaran_node_rows(self, nodes: Table, metrics: Table, assigned: Optional[Table], idx) -> Dict[str, np.ndarray]:
        """flatten_trimaran_nodes() for the listed nodes only (row j = node idx[j]): the input of update_trimaran_node_rows"""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        n = len(idx)
        cols = {
            "cap_cpu_milli": np.zeros(n, np.int64), "tlp_cpu_util": np.zeros(n, np.float64),
            "tlp_missing_milli": np.zeros(n, np.int64), "tlp_valid": np.zeros(n, np.uint8),
            "lv_alloc_cpu_milli": np.zeros(n, np.int64), "lv_alloc_mem": np.zeros(n, np.int64),
            "lv_cpu_avg": np.zeros(n, np.float64), "lv_cpu_std": np.zeros(n, np.float64),
            "lv_mem_avg": np.zeros(n, np.float64), "lv_mem_std": np.zeros(n, np.float64),
            "lv_flags": np.zeros(n, np.uint8),
        }
        fn = self._lib.spx_flatten_trimaran_node_rows
        ptrs = [v.ctypes.data_as(t) for v, t in zip(cols.values(), fn.argtypes[6:])]
        self._ck(fn(nodes.ref(), metrics.ref(), assigned.ref() if assigned else None, self.tlp_params.ref(),
                    idx.ctypes.data_as(C.POINTER(C.c_int64)), n, *ptrs))
        return cols

    def flatten_trimaran_pods(self, pods: Table) -> Dict[str, np.ndarray]:
        p = pods.struct.n_pods
        cols = {"tlp_pod_milli": np.zeros(p, np.int64), "lv_req_cpu_milli": np.zeros(p, np.int64),
                "lv_req_mem": np.zeros(p, np.int64)}
        i64p = C.POINTER(C.c_int64)
        self._ck(self._lib.spx_flatten_trimaran_pods(pods.ref(), self.tlp_params.ref(),
                                                      *[v.ctypes.data_as(i64p) for v in cols.values()]))
        return cols

    def upload_alloc_nodes(self, alloc: np.ndarray) -> None:
        alloc = np.ascontiguousarray(alloc, dtype=np.int64)
        t = Table(self._hdr, "spx_alloc_nodes_soa", n_nodes=alloc.shape[1], n_res=alloc.shape[0], alloc=alloc)
        self._ck(self._lib.spx_upload_alloc_nodes(self._h, t.ref()))
        self.n_nodes = alloc.shape[1]

    def upload_trimaran_nodes(self, cols: Dict[str, np.ndarray]) -> None:
        n = len(cols["cap_cpu_milli"])
        t = Table(self._hdr, "spx_trimaran_nodes_soa", n_nodes=n, **cols)
        self._ck(self._lib.spx_upload_trimaran_nodes(self._h, t.ref()))
        self.n_nodes = n

    def update_trimaran_nodes(self, idx, cols: Dict[str, np.ndarray]) -> None:
        """rows `idx` of the trimaran node table replaced in place: cols = flatten_trimaran_nodes()'s columns for ALL nodes, of
        which only rows idx travel (spx_update_trimaran_nodes)"""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        sub = {k: np.ascontiguousarray(v[idx]) for k, v in cols.items()}
        self._ck(self._lib.spx_update_trimaran_nodes(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                                     Table(self._hdr, "spx_trimaran_nodes_soa", n_nodes=len(idx), **sub).ref()))

    def update_trimaran_node_rows(self, idx, rows: Dict[str, np.ndarray]) -> None:
        """rows `idx` of the trimaran node table replaced in place: rows = flatten_trimaran_node_rows()'s columns (len(idx) rows)"""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        self._ck(self._lib.spx_update_trimaran_nodes(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                                     Table(self._hdr, "spx_trimaran_nodes_soa", n_nodes=len(idx), **rows).ref()))

    def update_nrt_nodes(self, idx, f: dict) -> None:
        """rows `idx` of the NRT node tables replaced in place: f = flatten_nrt()'s result for the NEW snapshot
        (spx_update_nrt_nodes; the derived float64 columns are recomputed on the device for those nodes)"""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        N, R = f["N"], f["R"]
        per = {"flags": 1, "max_numa": 1, "n_zones": 1, "zone_id": 8, "zone_present": 8, "zone_avail": 8 * max(R, 1), "zone_cost": 64,
               "min_avg_dist": 8, "node_present": 1}
        sub = {k: np.ascontiguousarray(f["nodes"][k].reshape(N, per[k])[idx].reshape(-1)) for k in per}
        self._ck(self._lib.spx_update_nrt_nodes(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                                Table(self._hdr, "spx_nrt_nodes_soa", n_nodes=len(idx), n_res=R, **sub).ref()))

    def upload_trimaran_pods(self, cols: Dict[str, np.ndarray], rows=None) -> None:
        cols = _rows(cols, len(cols["tlp_pod_milli"]), rows)
        p = len(cols["tlp_pod_milli"]) if rows is None else rows[1] - rows[0]
        if p > 0:
            t = Table(self._hdr, "spx_trimaran_pods_soa", n_pods=p, **cols)
            self._ck(self._lib.spx_upload_trimaran_pods(self._h, t.ref()))
        self.n_pods = p

    def load_trimaran_objects(self, nodes: Table, rc: Optional[Table], pods: Table, metrics: Table,
                              assigned: Optional[Table] = None) -> None:
        """objects -> (host flatten) -> SoA -> HBM, for Allocatable + TLP + LVRB."""
        self.upload_alloc_nodes(self.flatten_alloc_nodes(nodes, rc))
        self.upload_trimaran_nodes(self.flatten_trimaran_nodes(nodes, metrics, assigned))
        self.upload_trimaran_pods(self.flatten_trimaran_pods(pods))

    # ------------------------------------------------------------------ LowRiskOverCommitment
    _LROC_COLS = ("req_cpu_milli", "req_mem", "lim_cpu_milli", "lim_mem")

    def flatten_lroc_nodes(self, nodes: Table, node_pods: Optional[Table]) -> Dict[str, np.ndarray]:
        cols = {k: np.zeros(nodes.struct.n_nodes, np.int64) for k in self._LROC_COLS}
        i64p = C.POINTER(C.c_int64)
        self._ck(self._lib.spx_flatten_lroc_nodes(nodes.ref(), node_pods.ref() if node_pods else None,
                                                   *[v.ctypes.data_as(i64p) for v in cols.values()]))
        return cols

    def flatten_lroc_pods(self, pods: Table) -> Dict[str, np.ndarray]:
        cols = {k: np.zeros(pods.struct.n_pods, np.int64) for k in self._LROC_COLS}
        i64p = C.POINTER(C.c_int64)
        self._ck(self._lib.spx_flatten_lroc_pods(pods.ref(), *[v.ctypes.data_as(i64p) for v in cols.values()]))
        return cols

    def upload_lroc_nodes(self, cols: Dict[str, np.ndarray]) -> None:
        t = Table(self._hdr, "spx_lroc_nodes_soa", n_nodes=len(cols["req_mem"]), **cols)
        self._ck(self._lib.spx_upload_lroc_nodes(self._h, t.ref()))

    def upload_lroc_pods(self, cols: Dict[str, np.ndarray], rows=None) -> None:
        cols = _rows(cols, len(cols["req_mem"]), rows)
        p = len(cols["req_mem"]) if rows is None else rows[1] - rows[0]
        if p > 0:
            t = Table(self._hdr, "spx_lroc_pods_soa", n_pods=p, **cols)
            self._ck(self._lib.spx_upload_lroc_pods(self._h, t.ref()))
        self.n_pods = p

    def load_lroc_objects(self, nodes: Table, node_pods: Optional[Table], pods: Table) -> None:
        """LowRiskOverCommitment's own tables; the trimaran node table (metrics, allocatable) must be loaded already."""
        self.upload_lroc_nodes(self.flatten_lroc_nodes(nodes, node_pods))
        self.upload_lroc_pods(self.flatten_lroc_pods(pods))

    # ------------------------------------------------------------------ Peaks
    def flatten_peaks(self, nodes: Table, metrics: Table, power_models: Optional[Table], pods: Table) -> dict:
        n, p = nodes.struct.n_nodes, pods.struct.n_pods
        cols = {"cap_cpu_milli": np.zeros(n, np.int64), "cpu_util": np.zeros(n, np.float64), "valid": np.zeros(n, np.uint8),
                "k1": np.zeros(n, np.float64), "k2": np.zeros(n, np.float64)}
        fn = self._lib.spx_flatten_peaks_nodes
        self._ck(fn(nodes.ref(), metrics.ref(), power_models.ref() if power_models else None,
                    *[v.ctypes.data_as(t) for v, t in zip(cols.values(), fn.argtypes[3:])]))
        cpu = np.zeros(p, np.int64)
        self._ck(self._lib.spx_flatten_peaks_pods(pods.ref(), cpu.ctypes.data_as(C.POINTER(C.c_int64))))
        return {"nodes": cols, "pods": {"cpu_milli": cpu}, "N": n, "P": p}

    def upload_peaks(self, f: dict, rows=None) -> None:
        pc = _rows(f["pods"], f["P"], rows)
        p = f["P"] if rows is None else rows[1] - rows[0]
        self._ck(self._lib.spx_upload_peaks_nodes(self._h, Table(self._hdr, "spx_peaks_nodes_soa", n_nodes=f["N"], **f["nodes"]).ref()))
        if p > 0:
            self._ck(self._lib.spx_upload_peaks_pods(self._h, Table(self._hdr, "spx_peaks_pods_soa", n_pods=p, **pc).ref()))
        self.peaks_soa = dict(f["nodes"], cpu_milli=pc["cpu_milli"][:p])
        self.n_nodes, self.n_pods = f["N"], p

    def load_peaks_objects(self, nodes: Table, metrics: Table, power_models: Optional[Table], pods: Table) -> None:
        self.upload_peaks(self.flatten_peaks(nodes, metrics, power_models, pods))

    # ------------------------------------------------------------------ SySched
    def flatten_sysched(self, objects: Table) -> dict:
        """spx_sysched_objects -> {"nodes": spx_sysched_nodes_soa columns, "pods": spx_sysched_pods_soa columns, "W", "N", "P", "S"}"""
        o = objects.struct
        n, p, s = o.n_nodes, o.n_pods, o.n_sets
        w, n_stale = C.c_int32(), C.c_int64()
        fn = self._lib.spx_flatten_sysched_nodes
        self._ck_static(fn(objects.ref(), 0, C.byref(w), C.byref(n_stale), *([None] * 7)))
        W, ns = int(w.value), int(n_stale.value)
        nodes = {"host_bits": np.zeros((W, n), np.uint64), "present": np.zeros(n, np.uint8), "n_resident": np.zeros(n, np.int32),
                 "resident_missing": np.zeros(n, np.int32), "stale_ptr": np.zeros(n + 1, np.int32), "stale_bit": np.zeros(max(ns, 1), np.int32),
                 "stale_count": np.zeros(max(ns, 1), np.int32)}
        self._ck_static(fn(objects.ref(), ns, C.byref(w), C.byref(n_stale), *[v.ctypes.data_as(t) for v, t in zip(nodes.values(), fn.argtypes[4:])]))
        nodes["stale_bit"], nodes["stale_count"] = nodes["stale_bit"][:ns], nodes["stale_count"][:ns]
        pods = {"set_bits": np.zeros((max(s, 1), W), np.uint64), "pod_set": np.zeros(max(p, 1), np.int32)}
        fp = self._lib.spx_flatten_sysched_pods
        self._ck_static(fp(objects.ref(), *[v.ctypes.data_as(t) for v, t in zip(pods.values(), fp.argtypes[1:])]))
        pods["set_bits"], pods["pod_set"] = pods["set_bits"][:s], pods["pod_set"][:p]
        return {"nodes": nodes, "pods": pods, "W": W, "N": n, "P": p, "S": s}

    @staticmethod
    def sysched_node_rows(nodes: Dict[str, np.ndarray], idx) -> Dict[str, np.ndarray]:
        """the rows `idx` of flattened SySched node columns, in the layout spx_update_sysched_nodes takes"""
        idx = np.asarray(idx, np.int64)
        ptr = nodes["stale_ptr"]
        lens = ptr[idx + 1] - ptr[idx]
        take = np.concatenate([np.arange(ptr[i], ptr[i + 1]) for i in idx]).astype(np.int64) if len(idx) else np.zeros(0, np.int64)
        return {"host_bits": np.ascontiguousarray(nodes["host_bits"][:, idx]), "present": nodes["present"][idx], "n_resident": nodes["n_resident"][idx],
                "resident_missing": nodes["resident_missing"][idx], "stale_ptr": np.concatenate([[0], np.cumsum(lens)]).astype(np.int32),
                "stale_bit": nodes["stale_bit"][take], "stale_count": nodes["stale_count"][take]}

    def upload_sysched_nodes(self, nodes: Dict[str, np.ndarray]) -> None:
        W, n = nodes["host_bits"].shape
        self._ck(self._lib.spx_upload_sysched_nodes(self._h, Table(self._hdr, "spx_sysched_nodes_soa", n_nodes=n, n_words=W, **nodes).ref()))
        self.n_nodes = n

    def update_sysched_nodes(self, idx, rows: Dict[str, np.ndarray]) -> None:
        """rows: sysched_node_rows(...) of the changed nodes `idx` (spx_update_sysched_nodes)"""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        W = rows["host_bits"].shape[0]
        t = Table(self._hdr, "spx_sysched_nodes_soa", n_nodes=len(idx), n_words=W, **rows)
        self._ck(self._lib.spx_update_sysched_nodes(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), t.ref()))

    def upload_sysched_pods(self, pods: Dict[str, np.ndarray]) -> None:
        s, W = pods["set_bits"].shape
        p = len(pods["pod_set"])
        self._ck(self._lib.spx_upload_sysched_pods(self._h, Table(self._hdr, "spx_sysched_pods_soa", n_pods=p, n_words=W, n_sets=s, **pods).ref()))
        self.n_pods = p

    def load_sysched_objects(self, objects: Table) -> None:
        """flatten + upload both SySched tables in one call (spx_load_sysched)"""
        self._ck(self._lib.spx_load_sysched(self._h, objects.ref()))
        self.n_nodes, self.n_pods = objects.struct.n_nodes, objects.struct.n_pods

    # ------------------------------------------------------------------ Coscheduling
    def flatten_cosched(self, nodes: Table, objects: Table) -> dict:
        """spx_node_objects + spx_cosched_objects -> the columns of spx_cosched_soa (spx_flatten_cosched_slots / _nodes / _groups)"""
        L, o = self._lib, objects.struct
        N, G, P = int(o.n_nodes), int(o.n_groups), int(o.n_pods)
        n_slots, slot_res = C.c_int32(), np.zeros(self._hdr.consts["SPX_COSCHED_MAX_SLOTS"], np.int32)
        i32, i64, u8, u32 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
        self._ck_static(L.spx_flatten_cosched_slots(objects.ref(), C.byref(n_slots), slot_res.ctypes.data_as(i32)))
        S = int(n_slots.value)
        left, present = np.zeros((S, max(N, 1)), np.int64), np.zeros(max(N, 1), np.uint8)
        self._ck_static(L.spx_flatten_cosched_nodes(nodes.ref(), objects.ref(), S, slot_res.ctypes.data_as(i32), left.ctypes.data_as(i64), present.ctypes.data_as(u8)))
        n_steps = C.c_int64()
        self._ck_static(L.spx_flatten_cosched_groups(nodes.ref(), objects.ref(), S, slot_res.ctypes.data_as(i32), 0, C.byref(n_steps), None, None, None, None, None))
        K = int(n_steps.value)
        req, mask, sptr = np.zeros((max(G, 1), S), np.int64), np.zeros(max(G, 1), np.uint32), np.zeros(G + 1, np.int32)
        snode, sadd = np.zeros(max(K, 1), np.int32), np.zeros((max(K, 1), S), np.int64)
        self._ck_static(L.spx_flatten_cosched_groups(nodes.ref(), objects.ref(), S, slot_res.ctypes.data_as(i32), K, C.byref(n_steps), req.ctypes.data_as(i64),
                                                     mask.ctypes.data_as(u32), sptr.ctypes.data_as(i32), snode.ctypes.data_as(i32), sadd.ctypes.data_as(i64)))
        g = lambda k: objects.array(k)[:G] if G else np.zeros(0, objects.array(k).dtype)
        return {"N": N, "G": G, "P": P, "S": S, "slot_res": slot_res[:S].copy(), "left_base": left[:, :N], "node_present": present[:N],
                "g_exists": g("g_exists"), "min_member": g("g_min_member"), "has_min_resources": g("g_has_min_resources"), "backed_off": g("g_backed_off"),
                "permitted": g("g_permitted"), "listed": g("g_listed"), "gated": g("g_gated"), "req": req[:G], "req_mask": mask[:G], "step_ptr": sptr,
                "step_node": snode[:K], "step_add": sadd[:K], "pod_group": objects.array("pod_group")[:P]}

    def cosched_table(self, f: dict) -> Table:
        cols = {k: np.ascontiguousarray(f[k]) for k in ("slot_res", "left_base", "node_present", "g_exists", "min_member", "has_min_resources", "backed_off", "permitted",
                                                         "listed", "gated", "req", "req_mask", "step_ptr", "step_node", "step_add", "pod_group")}
        return Table(self._hdr, "spx_cosched_soa", n_nodes=f["N"], n_slots=f["S"], n_groups=f["G"], n_pods=f["P"], **cols)

    def cosched_check(self, f: dict) -> int:
        """the slot whose sums reach 2^62 (spx_cosched_check), -1 when the table is within the device's int64 range"""
        bad = C.c_int32(-1)
        rc = self._lib.spx_cosched_check(self.cosched_table(f).ref(), C.byref(bad))
        if rc != 0 and bad.value < 0:
            self._ck_static(rc)
        return int(bad.value)

    def upload_cosched(self, f: dict) -> None:
        """flatten_cosched's columns to the device; every upload makes the gate stale (spx_upload_cosched)"""
        self._ck(self._lib.spx_upload_cosched(self._h, self.cosched_table(f).ref()))
        self.n_nodes, self.n_pods = f["N"], f["P"]
        self._cosched_shape = (f["G"], f["S"])

    def load_cosched_objects(self, nodes: Table, objects: Table) -> None:
        self.upload_cosched(self.flatten_cosched(nodes, objects))

    def cosched_gap(self, group_begin: int = 0, group_end: Optional[int] = None):
        """(pass_mask [G], open_mask [G], gap [G][n_slots]) of CheckClusterResource per group (spx_fetch_cosched_gap)"""
        G, S = getattr(self, "_cosched_shape", (0, 1))
        group_end = G if group_end is None else group_end
        n = group_end - group_begin
        pm, om, gap = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, S), np.int64)
        u32 = C.POINTER(C.c_uint32)
        self._ck(self._lib.spx_fetch_cosched_gap(self._h, group_begin, group_end, pm.ctypes.data_as(u32), om.ctypes.data_as(u32), gap.ctypes.data_as(C.POINTER(C.c_int64))))
        return pm, om, gap

    def cosched_less(self, objects: Table, priority, initial_attempt_ns, keys: Sequence[str], a: Sequence[int], b: Sequence[int]) -> np.ndarray:
        """Coscheduling.Less for the pairs (a[i], b[i]) of pending pods; keys[p] = pod p's "namespace/name" (spx_cosched_less)"""
        enc = [k.encode() for k in keys]
        ptr = np.zeros(len(enc) + 1, np.int64)
        ptr[1:] = np.cumsum([len(k) for k in enc])
        blob = np.frombuffer(b"".join(enc) + b"\0", np.uint8).copy()
        pr = np.ascontiguousarray(priority, dtype=np.int32)
        ts = np.ascontiguousarray(initial_attempt_ns, dtype=np.int64)
        a = np.ascontiguousarray(a, dtype=np.int64)
        b = np.ascontiguousarray(b, dtype=np.int64)
        out = np.zeros(len(a), np.uint8)
        i64 = C.POINTER(C.c_int64)
        self._ck_static(self._lib.spx_cosched_less(objects.ref(), pr.ctypes.data_as(C.POINTER(C.c_int32)), ts.ctypes.data_as(i64), ptr.ctypes.data_as(i64),
                                                   blob.ctypes.data_as(C.POINTER(C.c_uint8)), len(a), a.ctypes.data_as(i64), b.ctypes.data_as(i64),
                                                   out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out.astype(bool)

    # ------------------------------------------------------------------ NodeResourceTopologyMatch
    def load_nrt_objects(self, nodes: Table, nrt: Table, rc: Optional[Table], pods: Table, params: Table) -> None:
        """objects -> (host flatten: slots, node zone tables, pod request tables) -> HBM."""
        self.upload_nrt(self.flatten_nrt(nodes, nrt, rc, pods, params))

    def flatten_nrt(self, nodes: Table, nrt: Table, rc: Optional[Table], pods: Table, params: Table) -> dict:
        """the NRT tables of a snapshot: the dense form up to 8 resource slots, the wide one (flatten_nrt_wide, "wide" in the dict)
        above 8 or with the NRT_WIDE option set — the choice spx_load_nrt makes"""
        L, H = self._lib, self._hdr
        if self._h and self.get_option("NRT_WIDE"):  # (a host-only wrapper has no engine, hence no options)
            return self.flatten_nrt_wide(nodes, nrt, rc, pods, params)
        u8p, i32p, i64p, f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)
        n_res = C.c_int32()
        slot_res = np.zeros(8, np.int32)
        slot_flags = np.zeros(8, np.uint8)
        slot_weight = np.zeros(8, np.int64)
        rc_ = L.spx_flatten_nrt_slots(pods.ref(), nrt.ref(), rc.ref() if rc else None, params.ref(), C.byref(n_res),
                                      slot_res.ctypes.data_as(i32p), slot_flags.ctypes.data_as(u8p), slot_weight.ctypes.data_as(i64p))
        if rc_ == H.consts["SPX_ERR_ARG"] and self.nrt_slots_wide(nrt, rc, pods, params)[0] > 8:
            return self.flatten_nrt_wide(nodes, nrt, rc, pods, params)
        self._ck(rc_)
        R = n_res.value
        slots = Table(H, "spx_nrt_slots", n_res=R, slot_res=slot_res, slot_flags=slot_flags, slot_weight=slot_weight)
        N, P = nodes.struct.n_nodes, pods.struct.n_pods
        nc = dict(flags=np.zeros(N, np.uint8), max_numa=np.zeros(N, np.int32), n_zones=np.zeros(N, np.uint8),
                  zone_id=np.zeros(N * 8, np.uint8), zone_present=np.zeros(N * 8, np.uint8),
                  zone_avail=np.zeros(N * 8 * max(R, 1), np.int64), zone_cost=np.zeros(N * 64, np.int32),
                  min_avg_dist=np.zeros(N * 8, np.float32), node_present=np.zeros(N, np.uint8))
        fn = L.spx_flatten_nrt_nodes
        rc_ = fn(nodes.ref(), nrt.ref(), slots.ref(), *[v.ctypes.data_as(t) for v, t in zip(nc.values(), fn.argtypes[3:])])
        if rc_ != 0:
            self._raise_nrt_zones(nrt)
            self._ck(rc_)  # (another reason: the flattener's own code, as before)
        tall = self.flatten_nrt_tall_nodes(nodes, nrt, slots)
        pc = dict(qos=np.zeros(P, np.uint8), non_native=np.zeros(P, np.uint8), n_ctr=np.zeros(P, np.uint8),
                  ctr_kind=np.zeros(P * 8, np.uint8), ctr_present=np.zeros(P * 8, np.uint8),
                  ctr_req=np.zeros(P * 8 * max(R, 1), np.int64), pod_present=np.zeros(P, np.uint8),
                  pod_req=np.zeros(P * max(R, 1), np.int64))
        fn = L.spx_flatten_nrt_pods
        self._ck(fn(pods.ref(), rc.ref() if rc else None, slots.ref(), *[v.ctypes.data_as(t) for v, t in zip(pc.values(), fn.argtypes[3:])]))
        pc = NrtPods(pc)
        pc.long = self.flatten_nrt_long_pods(pods, rc, slots)
        return {"params": params, "slots": slots, "nodes": nc, "pods": pc, "long": pc.long, "tall": tall, "N": N, "P": P, "R": R}

    def _raise_nrt_zones(self, nrt: Table, wide: bool = False) -> None:
        """raises when a node's zone count is why a node flattener refused the snapshot, naming the node (spx_nrt_first_tall_node);
        returns when it is not, and the caller reports the flattener's own code"""
        from . import SpxError
        node, nz = C.c_int64(), C.c_int32()
        rc = self._lib.spx_nrt_first_tall_node(nrt.ref(), C.byref(node), C.byref(nz))
        err = self._hdr.consts["SPX_ERR_ARG"]
        if rc != 0 and node.value >= 0:
            raise SpxError(err, f"NRT: node {node.value} lists {nz.value} NUMA zones of type Node (or one with id 64); this build takes up to 64 zones with ids 0..63")
        if wide and node.value >= 0:
            raise SpxError(err, f"NRT: node {node.value} lists {nz.value} NUMA zones; a wide snapshot (more than 8 resource slots, or the NRT_WIDE option) takes up to 8 per node")

    def nrt_slots_wide(self, nrt: Table, rc: Optional[Table], pods: Table, params: Table, cap: int = 32):
        """(count, status, slot_res, slot_flags, slot_weight) of spx_flatten_nrt_slots_wide with `cap` slots; the count is the snapshot's
        even when it exceeds cap (status SPX_ERR_ARG, arrays untouched)"""
        n_res = C.c_int32()
        slot_res, slot_flags, slot_weight = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.int64)
        st = self._lib.spx_flatten_nrt_slots_wide(pods.ref(), nrt.ref(), rc.ref() if rc else None, params.ref(), cap, C.byref(n_res),
                                                  slot_res.ctypes.data_as(C.POINTER(C.c_int32)), slot_flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                  slot_weight.ctypes.data_as(C.POINTER(C.c_int64)))
        return n_res.value, st, slot_res, slot_flags, slot_weight

    def flatten_nrt_wide(self, nodes: Table, nrt: Table, rc: Optional[Table], pods: Table, params: Table) -> dict:
        """the wide NRT tables (up to 32 resource slots): slots, nodes (spx_nrt_nodes_wide columns) and pods (spx_nrt_pods_wide columns)"""
        L, H = self._lib, self._hdr
        R, st, slot_res, slot_flags, slot_weight = self.nrt_slots_wide(nrt, rc, pods, params)
        if st != 0:
            from . import SpxError
            raise SpxError(st,f"NRT: the snapshot names {R} distinct resources; this build takes up to 32" if R > 32 else "spx_flatten_nrt_slots_wide failed")
        slots = Table(H, "spx_nrt_slots", n_res=R, slot_res=slot_res, slot_flags=slot_flags, slot_weight=slot_weight)
        N, P = nodes.struct.n_nodes, pods.struct.n_pods
        nc = dict(flags=np.zeros(N, np.uint8), max_numa=np.zeros(N, np.int32), n_zones=np.zeros(N, np.uint8),
                  zone_id=np.zeros(N * 8, np.uint8), zone_present=np.zeros(N * 8, np.uint32),
                  zone_avail=np.zeros(N * 8 * max(R, 1), np.int64), zone_cost=np.zeros(N * 64, np.int32),
                  min_avg_dist=np.zeros(N * 8, np.float32), node_present=np.zeros(N, np.uint32))
        fn = L.spx_flatten_nrt_nodes_wide
        rc_ = fn(nodes.ref(), nrt.ref(), slots.ref(), *[v.ctypes.data_as(t) for v, t in zip(nc.values(), fn.argtypes[3:])])
        if rc_ != 0:
            self._raise_nrt_zones(nrt, wide=True)
            self._ck_static(rc_)
        return {"wide": True, "params": params, "slots": slots, "nodes": nc, "pods": self.flatten_nrt_pods_wide(pods, rc, slots),
                "N": N, "P": P, "R": R}

    def flatten_nrt_pods_wide(self, pods: Table, rc: Optional[Table], slots: Table) -> Dict[str, np.ndarray]:
        """the wide pod table (spx_flatten_nrt_pods_wide): CSR lists of (slot, quantity), pod-level and per container"""
        L = self._lib
        P = pods.struct.n_pods
        cptr = pods.array("ctr_ptr")
        n_ctr = int(cptr[P]) - int(cptr[0])  # (a pod view may start inside a larger table)
        args = (pods.ref(), rc.ref() if rc else None, slots.ref())
        n_req, n_ent = C.c_int64(), C.c_int64()
        self._ck_static(L.spx_flatten_nrt_pods_wide(*args, 0, 0, C.byref(n_req), C.byref(n_ent), *([None] * 10)))
        nr, ne = n_req.value, n_ent.value
        pw = dict(qos=np.zeros(P, np.uint8), non_native=np.zeros(P, np.uint8), req_ptr=np.zeros(P + 1, np.int32), req_slot=np.zeros(nr, np.uint8),
                  req_qty=np.zeros(nr, np.int64), ctr_ptr=np.zeros(P + 1, np.int32), ctr_kind=np.zeros(n_ctr, np.uint8),
                  ent_ptr=np.zeros(n_ctr + 1, np.int32), ent_slot=np.zeros(ne, np.uint8), ent_qty=np.zeros(ne, np.int64))
        fn = L.spx_flatten_nrt_pods_wide
        self._ck_static(fn(*args, nr, ne, C.byref(n_req), C.byref(n_ent),
                           *[pw[k].ctypes.data_as(t) for k, t in zip(WIDE_POD_COLS, fn.argtypes[7:])]))
        return pw

    def nrt_wide(self) -> bool:
        """whether the NRT tables in place are the wide form (spx_nrt_wide)"""
        return bool(self._lib.spx_nrt_wide(self._h))

    def flatten_nrt_long_pods(self, pods: Table, rc: Optional[Table], slots: Table) -> dict:
        """the containers of the pods with more than 8 containers, CSR (spx_flatten_nrt_long_pods): n_long, pod_row, ctr_ptr,
        ctr_kind, ctr_present, ctr_req [n_ctr * n_res]"""
        L = self._lib
        R = int(slots.struct.n_res)
        n_long, n_ctr = C.c_int64(), C.c_int64()
        args = (pods.ref(), rc.ref() if rc else None, slots.ref())
        self._ck_static(L.spx_flatten_nrt_long_pods(*args, 0, 0, C.byref(n_long), C.byref(n_ctr), None, None, None, None, None))
        nl, nc = n_long.value, n_ctr.value
        lt = dict(n_long=nl, pod_row=np.zeros(nl, np.int32), ctr_ptr=np.zeros(nl + 1, np.int32), ctr_kind=np.zeros(nc, np.uint8),
                  ctr_present=np.zeros(nc, np.uint8), ctr_req=np.zeros(nc * max(R, 1), np.int64))
        if nl:
            self._ck_static(L.spx_flatten_nrt_long_pods(*args, nl, nc, C.byref(n_long), C.byref(n_ctr),
                                                        *[lt[k].ctypes.data_as(t) for k, t in zip(("pod_row", "ctr_ptr", "ctr_kind", "ctr_present", "ctr_req"),
                                                                                                  L.spx_flatten_nrt_long_pods.argtypes[7:])]))
        return lt

    def upload_nrt_long_pods(self, lt: Optional[dict], n_res: int) -> None:
        """the long rows' containers (spx_upload_nrt_long_pods), after the pod table they belong to; None = an empty table"""
        if lt is None:
            lt = dict(n_long=0)
        cols = {k: lt[k] for k in ("pod_row", "ctr_ptr", "ctr_kind", "ctr_present", "ctr_req") if k in lt and len(lt[k])}
        self._ck(self._lib.spx_upload_nrt_long_pods(self._h, Table(self._hdr, "spx_nrt_long_pods", n_long=int(lt["n_long"]), n_res=n_res, **cols).ref()))

    TALL_COLS = ("node_idx", "flags", "max_numa", "node_present", "n_zones", "zone_id", "zone_present", "zone_avail", "zone_cost", "min_avg_dist")

    def flatten_nrt_tall_nodes(self, nodes: Table, nrt: Table, slots: Table) -> dict:
        """the zones of the nodes with more than 8 NUMA zones (spx_flatten_nrt_tall_nodes): n_tall, zone_stride and the columns of
        spx_nrt_tall_nodes, host row-major (zone_id [n_tall * zone_stride], zone_avail [n_tall * zone_stride * n_res], ...)"""
        L = self._lib
        R = int(slots.struct.n_res)
        n_tall, zs = C.c_int64(), C.c_int32()
        args = (nodes.ref(), nrt.ref(), slots.ref())
        rc_ = L.spx_flatten_nrt_tall_nodes(*args, 0, 0, C.byref(n_tall), C.byref(zs), *([None] * 10))
        if rc_ != 0:
            self._raise_nrt_zones(nrt)
            self._ck_static(rc_)
        T, S = n_tall.value, zs.value
        tt = dict(n_tall=T, zone_stride=S, node_idx=np.zeros(T, np.int32), flags=np.zeros(T, np.uint8), max_numa=np.zeros(T, np.int32),
                  node_present=np.zeros(T, np.uint8), n_zones=np.zeros(T, np.uint8), zone_id=np.zeros(T * S, np.uint8),
                  zone_present=np.zeros(T * S, np.uint8), zone_avail=np.zeros(T * S * max(R, 1), np.int64),
                  zone_cost=np.zeros(T * S * S, np.int32), min_avg_dist=np.zeros(T * S, np.float32))
        if T:
            fn = L.spx_flatten_nrt_tall_nodes
            self._ck_static(fn(*args, T, S, C.byref(n_tall), C.byref(zs), *[tt[k].ctypes.data_as(t) for k, t in zip(self.TALL_COLS, fn.argtypes[7:])]))
        return tt

    def upload_nrt_tall_nodes(self, tt: Optional[dict], n_res: int) -> None:
        """the tall nodes' zones (spx_upload_nrt_tall_nodes), after the node table they belong to; None = an empty table"""
        if tt is None:
            tt = dict(n_tall=0, zone_stride=0)
        cols = {k: tt[k] for k in self.TALL_COLS if k in tt and len(tt[k])}
        self._ck(self._lib.spx_upload_nrt_tall_nodes(self._h, Table(self._hdr, "spx_nrt_tall_nodes", n_tall=int(tt["n_tall"]), n_res=n_res,
                                                                    zone_stride=int(tt.get("zone_stride", 0)), **cols).ref()))

    def nrt_tall_nodes(self) -> int:
        """tall nodes (more than 8 NUMA zones) the last NRT sweep of eval evaluated (spx_nrt_tall_count)"""
        n = C.c_int64()
        self._ck(self._lib.spx_nrt_tall_count(self._h, C.byref(n)))
        return n.value

    def nrt_long_rows(self) -> int:
        """long rows (pods with more than 8 containers) the last NRT sweep of eval evaluated (spx_nrt_long_rows)"""
        n = C.c_int64()
        self._ck(self._lib.spx_nrt_long_rows(self._h, C.byref(n)))
        return n.value

    def flatten_nrt_node_rows(self, nodes: Table, nrt: Table, slots: Table, idx) -> Dict[str, np.ndarray]:
        """the SoA rows of the listed nodes only (spx_flatten_nrt_node_rows): what a delta encoder produces for the changed nodes"""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        n, R = len(idx), int(slots.struct.n_res)
        nc = dict(flags=np.zeros(n, np.uint8), max_numa=np.zeros(n, np.int32), n_zones=np.zeros(n, np.uint8),
                  zone_id=np.zeros(n * 8, np.uint8), zone_present=np.zeros(n * 8, np.uint8),
                  zone_avail=np.zeros(n * 8 * max(R, 1), np.int64), zone_cost=np.zeros(n * 64, np.int32),
                  min_avg_dist=np.zeros(n * 8, np.float32), node_present=np.zeros(n, np.uint8))
        fn = self._lib.spx_flatten_nrt_node_rows
        self._ck(fn(nodes.ref(), nrt.ref(), slots.ref(), idx.ctypes.data_as(C.POINTER(C.c_int64)), n,
                    *[v.ctypes.data_as(t) for v, t in zip(nc.values(), fn.argtypes[5:])]))
        return nc

    def update_nrt_node_rows(self, idx, rows: Dict[str, np.ndarray], n_res: int) -> None:
        """spx_update_nrt_nodes with rows as flatten_nrt_node_rows returns them"""
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        self._ck(self._lib.spx_update_nrt_nodes(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                                Table(self._hdr, "spx_nrt_nodes_soa", n_nodes=len(idx), n_res=n_res, **rows).ref()))

    def flatten_nrt_pods(self, pods: Table, rc: Optional[Table], slots: Table) -> Dict[str, np.ndarray]:
        """the pod half of flatten_nrt for a NEW pending batch against slots already uploaded (a cycle's pod delta)"""
        u8p, i64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int64)
        P, R = pods.struct.n_pods, int(slots.struct.n_res)
        pc = dict(qos=np.zeros(P, np.uint8), non_native=np.zeros(P, np.uint8), n_ctr=np.zeros(P, np.uint8),
                  ctr_kind=np.zeros(P * 8, np.uint8), ctr_present=np.zeros(P * 8, np.uint8),
                  ctr_req=np.zeros(P * 8 * max(R, 1), np.int64), pod_present=np.zeros(P, np.uint8),
                  pod_req=np.zeros(P * max(R, 1), np.int64))
        fn = self._lib.spx_flatten_nrt_pods
        self._ck(fn(pods.ref(), rc.ref() if rc else None, slots.ref(), *[v.ctypes.data_as(t) for v, t in zip(pc.values(), fn.argtypes[3:])]))
        pc = NrtPods(pc)
        pc.long = self.flatten_nrt_long_pods(pods, rc, slots)
        return pc

    def set_nrt_params(self, params: Table) -> None:
        """the scoring strategy alone (spx_set_nrt_params): slot weights travel with the slot table, the tables stay in place"""
        self._ck(self._lib.spx_set_nrt_params(self._h, params.ref()))

    def upload_nrt_nodes(self, nc: Dict[str, np.ndarray], n_res: int) -> None:
        """the node zone tables alone, for the pod batch in place (spx_upload_nrt_nodes: the preemption dry run's re-upload)"""
        n = len(nc["flags"])
        self._ck(self._lib.spx_upload_nrt_nodes(self._h, Table(self._hdr, "spx_nrt_nodes_soa", n_nodes=n, n_res=n_res, **nc).ref()))
        self.n_nodes = n
        if getattr(self, "nrt_soa", None) is not None:
            self.nrt_soa["nodes"] = nc

    def upload_nrt_pods(self, pc: Dict[str, np.ndarray], n_res: int) -> None:
        P = len(pc["qos"])
        self._ck(self._lib.spx_upload_nrt_pods(self._h, Table(self._hdr, "spx_nrt_pods_soa", n_pods=P, n_res=n_res, **pc).ref()))
        if getattr(pc, "long", None) is not None:
            self.upload_nrt_long_pods(pc.long, n_res)
        self.n_pods = P
        self.nrt_soa["pods"] = pc

    def flatten_network_pods(self, pods: Table, appgroups: Table) -> dict:
        """the per-batch half of flatten_network (workload keys of the pending pods), without the commit effects"""
        L = self._lib
        i32p, i64p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
        P = pods.struct.n_pods
        nk, npairs = C.c_int32(), C.c_int64()
        self._ck(L.spx_flatten_net_keys(pods.ref(), appgroups.ref(), C.byref(nk), C.byref(npairs), None, None, None, None, None, None))
        cols = dict(pod_key=np.zeros(P, np.int32), topo_order=np.zeros(P, np.int32), key_score_equally=np.zeros(nk.value, np.uint8),
                    pair_ptr=np.zeros(nk.value + 1, np.int32), pair_node=np.zeros(max(npairs.value, 1), np.int32),
                    pair_max_cost=np.zeros(max(npairs.value, 1), np.int64))
        self._ck(L.spx_flatten_net_keys(pods.ref(), appgroups.ref(), C.byref(nk), C.byref(npairs),
                                        cols["pod_key"].ctypes.data_as(i32p), cols["topo_order"].ctypes.data_as(i32p),
                                        cols["key_score_equally"].ctypes.data_as(u8p), cols["pair_ptr"].ctypes.data_as(i32p),
                                        cols["pair_node"].ctypes.data_as(i32p), cols["pair_max_cost"].ctypes.data_as(i64p)))
        return {"cols": cols, "n_keys": nk.value, "P": P}

    def upload_network_pods(self, f: dict) -> None:
        self._ck(self._lib.spx_upload_net_pods(self._h, Table(self._hdr, "spx_net_pods_soa", n_pods=f["P"], n_keys=f["n_keys"], **f["cols"]).ref()))
        self.n_pods = f["P"]
        self.net_soa = f["cols"]

    def flatten_net_placed(self, pods: Table, appgroups: Table, group, selector, node) -> dict:
        """pods that joined AppGroup scheduled lists since flatten_network_pods(pods, appgroups): the entries update_net_placed appends"""
        L = self._lib
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        g, sel, nd = (np.ascontiguousarray(x, dtype=np.int32) for x in (group, selector, node))
        n = C.c_int64()
        args = (pods.ref(), appgroups.ref(), len(g), g.ctypes.data_as(i32p), sel.ctypes.data_as(i32p), nd.ctypes.data_as(i32p), C.byref(n))
        self._ck_static(L.spx_flatten_net_placed(*args, None, None, None))
        out = dict(key=np.zeros(max(n.value, 1), np.int32), node=np.zeros(max(n.value, 1), np.int32), max_cost=np.zeros(max(n.value, 1), np.int64))
        self._ck_static(L.spx_flatten_net_placed(*args, out["key"].ctypes.data_as(i32p), out["node"].ctypes.data_as(i32p), out["max_cost"].ctypes.data_as(i64p)))
        return {k: v[:n.value] for k, v in out.items()}

    def update_net_placed(self, ent: dict) -> None:
        """the workload keys' pair lists grown in place on the device (spx_update_net_placed)"""
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        k, nd, c = np.ascontiguousarray(ent["key"], np.int32), np.ascontiguousarray(ent["node"], np.int32), np.ascontiguousarray(ent["max_cost"], np.int64)
        self._ck(self._lib.spx_update_net_placed(self._h, len(k), k.ctypes.data_as(i32p), nd.ctypes.data_as(i32p), c.ctypes.data_as(i64p)))

    def update_quota_used(self, ns, used, used_present, agg_used, agg_used_present) -> None:
        """rows `ns` of ElasticQuotaInfo.Used replaced in place, with the new aggregate (spx_update_quota_used)"""
        i32p, i64p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
        ns = np.ascontiguousarray(ns, np.int32)
        used = np.ascontiguousarray(used, np.int64).reshape(-1)
        up, au, aup = np.ascontiguousarray(used_present, np.uint8), np.ascontiguousarray(agg_used, np.int64), np.ascontiguousarray(agg_used_present, np.uint8).reshape(-1)
        assert used.size == len(ns) * 8 and au.size == 8
        self._ck(self._lib.spx_update_quota_used(self._h, len(ns), ns.ctypes.data_as(i32p), used.ctypes.data_as(i64p), up.ctypes.data_as(u8p),
                                                 au.ctypes.data_as(i64p), aup.ctypes.data_as(u8p)))

    def upload_nrt(self, f: dict, rows=None) -> None:
        """rows = (begin, end): this engine holds only that slice of the pod batch (MultiEngine)"""
        L, H = self._lib, self._hdr
        if f.get("wide"):
            self._ck(L.spx_set_nrt_params(self._h, f["params"].ref()))
            self._ck(L.spx_upload_nrt_slots_wide(self._h, f["slots"].ref()))
            self._ck(L.spx_upload_nrt_nodes_wide(self._h, Table(H, "spx_nrt_nodes_wide", n_nodes=f["N"], n_res=f["R"], **f["nodes"]).ref()))
            pw = wide_rows_slice(f["pods"], rows)
            P = f["P"] if rows is None else rows[1] - rows[0]
            if P > 0:
                cols = {k: v for k, v in pw.items() if len(v)}  # (an empty list column travels as NULL)
                self._ck(L.spx_upload_nrt_pods_wide(self._h, Table(H, "spx_nrt_pods_wide", n_pods=P, n_res=f["R"], **cols).ref()))
            self.n_nodes, self.n_pods = f["N"], P
            self.nrt_soa = {"slots": f["slots"], "nodes": f["nodes"], "pods": pw, "wide": True}
            return
        self._ck(L.spx_set_nrt_params(self._h, f["params"].ref()))
        self._ck(L.spx_upload_nrt_slots(self._h, f["slots"].ref()))
        self._ck(L.spx_upload_nrt_nodes(self._h, Table(H, "spx_nrt_nodes_soa", n_nodes=f["N"], n_res=f["R"], **f["nodes"]).ref()))
        if f.get("tall") is not None:
            self.upload_nrt_tall_nodes(f["tall"], f["R"])
        pc = _rows(f["pods"], f["P"], rows)
        P = f["P"] if rows is None else rows[1] - rows[0]
        if P > 0:
            self._ck(L.spx_upload_nrt_pods(self._h, Table(H, "spx_nrt_pods_soa", n_pods=P, n_res=f["R"], **pc).ref()))
            lt = f.get("long", getattr(f["pods"], "long", None))
            if lt is not None:
                self.upload_nrt_long_pods(long_rows_slice(lt, rows, f["R"]), f["R"])
        self.n_nodes, self.n_pods = f["N"], P
        self.nrt_soa = {"slots": f["slots"], "nodes": f["nodes"], "pods": pc}

    # ------------------------------------------------------------------ NetworkOverhead / TopologicalSort
    def load_network_objects(self, nodes: Table, pods: Table, appgroups: Table, nettopo: Table) -> None:
        self.upload_network(self.flatten_network(nodes, pods, appgroups, nettopo))

    def flatten_network(self, nodes: Table, pods: Table, appgroups: Table, nettopo: Table) -> dict:
        L, H = self._lib, self._hdr
        i32p, i64p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
        N, P = nodes.struct.n_nodes, pods.struct.n_pods
        rg, zc = nettopo.struct.n_regions, nettopo.struct.n_zones
        # the cost matrices in the CRD's own int64; a snapshot whose entries all fit int32 is narrowed and travels as before
        rcost = np.full(max(rg * rg, 1), -1, np.int64)
        zcost = np.full(max(zc * zc, 1), -1, np.int64)
        self._ck(L.spx_flatten_net_topo_wide(nettopo.ref(), rcost.ctypes.data_as(i64p), zcost.ctypes.data_as(i64p)))
        if max(rcost.max(), zcost.max()) <= np.iinfo(np.int32).max:
            rcost, zcost = rcost.astype(np.int32), zcost.astype(np.int32)
        nk, npairs = C.c_int32(), C.c_int64()
        self._ck(L.spx_flatten_net_keys(pods.ref(), appgroups.ref(), C.byref(nk), C.byref(npairs), None, None, None, None, None, None))
        cols = dict(pod_key=np.zeros(P, np.int32), topo_order=np.zeros(P, np.int32), key_score_equally=np.zeros(nk.value, np.uint8),
                    pair_ptr=np.zeros(nk.value + 1, np.int32), pair_node=np.zeros(max(npairs.value, 1), np.int32),
                    pair_max_cost=np.zeros(max(npairs.value, 1), np.int64))
        self._ck(L.spx_flatten_net_keys(pods.ref(), appgroups.ref(), C.byref(nk), C.byref(npairs),
                                        cols["pod_key"].ctypes.data_as(i32p), cols["topo_order"].ctypes.data_as(i32p),
                                        cols["key_score_equally"].ctypes.data_as(u8p), cols["pair_ptr"].ctypes.data_as(i32p),
                                        cols["pair_node"].ctypes.data_as(i32p), cols["pair_max_cost"].ctypes.data_as(i64p)))
        # what binding each pod adds to the AppGroup scheduled lists (sequential commit loop)
        n_eff = C.c_int64()
        self._ck(L.spx_flatten_net_commit(pods.ref(), appgroups.ref(), C.byref(n_eff), None, None, None))
        eff = dict(eff_ptr=np.zeros(P + 1, np.int32), eff_key=np.zeros(max(n_eff.value, 1), np.int32), eff_max_cost=np.zeros(max(n_eff.value, 1), np.int64))
        self._ck(L.spx_flatten_net_commit(pods.ref(), appgroups.ref(), C.byref(n_eff), eff["eff_ptr"].ctypes.data_as(i32p),
                                          eff["eff_key"].ctypes.data_as(i32p), eff["eff_max_cost"].ctypes.data_as(i64p)))
        return {"region": nodes.array("region"), "zone": nodes.array("zone"), "rg": rg, "zc": zc, "rcost": rcost, "zcost": zcost,
                "n_keys": nk.value, "cols": cols, "N": N, "P": P, "commit": eff}

    def upload_network(self, f: dict, rows=None) -> None:
        L, H = self._lib, self._hdr
        self._ck(L.spx_upload_net_nodes(self._h, Table(H, "spx_net_nodes_soa", n_nodes=f["N"], region=f["region"], zone=f["zone"]).ref()))
        if f["rcost"].dtype == np.int64:  # int64 cost matrices: the wide tables (the engine then runs its 64-bit sweep)
            self._ck(L.spx_upload_net_topo_wide(self._h, Table(H, "spx_net_topo_wide", n_regions=f["rg"], n_zones=f["zc"], region_cost=f["rcost"],
                                                                zone_cost=f["zcost"]).ref()))
        else:
            self._ck(L.spx_upload_net_topo(self._h, Table(H, "spx_net_topo_soa", n_regions=f["rg"], n_zones=f["zc"], region_cost=f["rcost"],
                                                           zone_cost=f["zcost"]).ref()))
        cols = dict(f["cols"])
        P = f["P"] if rows is None else rows[1] - rows[0]
        cols.update(_rows({k: cols[k] for k in ("pod_key", "topo_order")}, f["P"], rows))  # the key tables are per workload, not per pod
        if P > 0:
            self._ck(L.spx_upload_net_pods(self._h, Table(H, "spx_net_pods_soa", n_pods=P, n_keys=f["n_keys"], **cols).ref()))
            if rows is None:  # the commit effects index the whole batch
                self._ck(L.spx_upload_net_commit(self._h, Table(H, "spx_net_commit_soa", n_pods=P, **f["commit"]).ref()))
        self.n_nodes, self.n_pods = f["N"], P
        self.net_soa = cols

    # ---- NodeMetadata / PodState / QOSSort
    @staticmethod
    def _static_lib():
        from . import lib
        return lib()

    @staticmethod
    def _static_fail(rc: int, msg: str):
        from . import SpxError
        return SpxError(rc, msg)

    @classmethod
    def flatten_nodemeta(cls, values: Sequence[Optional[object]], mtype: str = "Number", strategy: str = "Highest", now_unix_nanos: int = 0) -> np.ndarray:
        """the node's label or annotation strings (None = key not found) -> NodeMetadata's raw int64 column (spx_flatten_nodemeta)"""
        enc = [b"" if v is None else (v if isinstance(v, bytes) else str(v).encode()) for v in values]
        ptr = np.zeros(len(enc) + 1, np.int64)
        np.cumsum([len(b) for b in enc], out=ptr[1:])
        blob = b"".join(enc) + b"\0"
        found = np.array([v is not None for v in values], np.uint8)
        out = np.zeros(len(enc), np.int64)
        if len(enc) == 0:
            return out
        rc = cls._static_lib().spx_flatten_nodemeta(blob, ptr.ctypes.data_as(C.POINTER(C.c_int64)), found.ctypes.data_as(C.POINTER(C.c_uint8)), len(enc),
                                                    NODEMETA_TYPE[mtype], NODEMETA_STRATEGY[strategy], now_unix_nanos, out.ctypes.data_as(C.POINTER(C.c_int64)))
        if rc != 0:
            raise cls._static_fail(rc, "spx_flatten_nodemeta: invalid argument")
        return out

    @classmethod
    def flatten_nodemeta_unix(cls, unix_nanos, valid, strategy: str = "Newest", now_unix_nanos: int = 0) -> np.ndarray:
        """timestamps the caller parsed (any TimestampFormat) -> the raw column (spx_flatten_nodemeta_unix)"""
        t = np.ascontiguousarray(unix_nanos, dtype=np.int64)
        v = np.ascontiguousarray(valid, dtype=np.uint8)
        out = np.zeros(len(t), np.int64)
        rc = cls._static_lib().spx_flatten_nodemeta_unix(t.ctypes.data_as(C.POINTER(C.c_int64)), v.ctypes.data_as(C.POINTER(C.c_uint8)), len(t),
                                                         NODEMETA_STRATEGY[strategy], now_unix_nanos, out.ctypes.data_as(C.POINTER(C.c_int64)))
        if rc != 0:
            raise cls._static_fail(rc, "spx_flatten_nodemeta_unix: invalid argument")
        return out

    @classmethod
    def flatten_podstate(cls, n_nodes: int, assigned_node, assigned_terminating, nominated_node) -> np.ndarray:
        """terminating minus nominated pods per node (spx_flatten_podstate)"""
        an = np.ascontiguousarray(assigned_node, dtype=np.int64)
        at = np.ascontiguousarray(assigned_terminating, dtype=np.uint8)
        nn = np.ascontiguousarray(nominated_node, dtype=np.int64)
        out = np.zeros(max(n_nodes, 0), np.int64)
        i64p = C.POINTER(C.c_int64)
        rc = cls._static_lib().spx_flatten_podstate(n_nodes, len(an), an.ctypes.data_as(i64p), at.ctypes.data_as(C.POINTER(C.c_uint8)), len(nn),
                                                    nn.ctypes.data_as(i64p), out.ctypes.data_as(i64p))
        if rc != 0:
            raise cls._static_fail(rc, "spx_flatten_podstate: a node index outside [0, n_nodes), or a NULL column")
        return out

    @classmethod
    def flatten_pod_qos(cls, pods: Table) -> np.ndarray:
        """v1qos.GetPodQOS per pod in QOSSort's numbering: 1 BestEffort, 2 Burstable, 3 Guaranteed (spx_flatten_pod_qos)"""
        out = np.zeros(pods.struct.n_pods, np.uint8)
        rc = cls._static_lib().spx_flatten_pod_qos(pods.ref(), out.ctypes.data_as(C.POINTER(C.c_uint8)))
        if rc != 0:
            raise cls._static_fail(rc, "spx_flatten_pod_qos: invalid argument")
        return out

    @classmethod
    def qos_less(cls, priority1: int, qos1: int, ts1: int, priority2: int, qos2: int, ts2: int) -> bool:
        """QOSSort's Less for one pair (spx_qos_less)"""
        return bool(cls._static_lib().spx_qos_less(priority1, qos1, ts1, priority2, qos2, ts2))

    def upload_nodemeta(self, raw) -> None:
        """NodeMetadata's raw column, INVALID_SCORE = no valid metadata (spx_upload_nodemeta_nodes)"""
        raw = np.ascontiguousarray(raw, dtype=np.int64)
        self._ck(self._lib.spx_upload_nodemeta_nodes(self._h, Table(self._hdr, "spx_node_column_soa", n_nodes=len(raw), raw=raw).ref(), 0))
        self.n_nodes = len(raw)

    def upload_podstate(self, raw) -> None:
        """PodState's raw column: terminating minus nominated pods per node (spx_upload_podstate_nodes)"""
        raw = np.ascontiguousarray(raw, dtype=np.int64)
        self._ck(self._lib.spx_upload_podstate_nodes(self._h, Table(self._hdr, "spx_node_column_soa", n_nodes=len(raw), raw=raw).ref()))
        self.n_nodes = len(raw)

    def upload_qos_sort_keys(self, priority, qos, queue_ts) -> None:
        priority = np.ascontiguousarray(priority, dtype=np.int32)
        t = Table(self._hdr, "spx_qos_sort_keys_soa", n_pods=len(priority), priority=priority, qos=qos, queue_ts=queue_ts)
        self._ck(self._lib.spx_upload_qos_sort_keys(self._h, t.ref()))
        self._qos_n = len(priority)

    def qos_sort(self) -> np.ndarray:
        """QOSSort as one device sort: the queue order as pod rows (spx_qos_sort)"""
        perm = np.zeros(getattr(self, "_qos_n", 0) or 1, np.int32)
        self._ck(self._lib.spx_qos_sort(self._h, perm.ctypes.data_as(C.POINTER(C.c_int32))))
        return perm[:getattr(self, "_qos_n", 0)]

    def sort_queue(self, pods: Table, topo_order: Optional[np.ndarray] = None) -> np.ndarray:
        """TopologicalSort as one device sort: queue order (pod rows) in which every adjacent pair satisfies Less (spx_sort_keys)"""
        topo = np.ascontiguousarray(self.net_soa["topo_order"] if topo_order is None else topo_order, dtype=np.int32)
        n = pods.struct.n_pods
        t = Table(self._hdr, "spx_sort_keys_soa", n_pods=n, priority=pods.array("priority"), queue_ts=pods.array("queue_ts"),
                  appgroup=pods.array("appgroup"), topo_order=topo)
        self._ck(self._lib.spx_upload_sort_keys(self._h, t.ref()))
        perm = np.zeros(n, np.int32)
        self._ck(self._lib.spx_sort_keys(self._h, perm.ctypes.data_as(C.POINTER(C.c_int32))))
        return perm

    def toposort_less(self, pods: Table, a: Sequence[int], b: Sequence[int]) -> np.ndarray:
        a = np.ascontiguousarray(a, dtype=np.int64)
        b = np.ascontiguousarray(b, dtype=np.int64)
        out = np.zeros(len(a), np.uint8)
        i64p = C.POINTER(C.c_int64)
        self._ck_static(self._lib.spx_toposort_less(pods.ref(), self.net_soa["topo_order"].ctypes.data_as(C.POINTER(C.c_int32)), len(a),
                                                    a.ctypes.data_as(i64p), b.ctypes.data_as(i64p),
                                                    out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out.astype(bool)

    @staticmethod
    def _ck_static(rc: int) -> None:
        if rc != 0:
            raise RuntimeError(f"spx host call failed: {rc}")

    # ------------------------------------------------------------------ CapacityScheduling.PreFilter
    def load_quota_objects(self, pods: Table, rc: Optional[Table], quota: Table) -> None:
        self.upload_quota(self.flatten_quota(pods, rc, quota))

    def flatten_quota(self, pods: Table, rc: Optional[Table], quota: Table) -> dict:
        L, H = self._lib, self._hdr
        P, NS = pods.struct.n_pods, quota.struct.n_namespaces
        nn = max(int(quota.struct.n_nominated), 1)
        cols = dict(pod_ns=np.zeros(P, np.int32), pod_priority=np.zeros(P, np.int32), pod_req=np.zeros(P * 8, np.int64),
                    pod_req_present=np.zeros(P, np.uint8), agg_used=np.zeros(8, np.int64), agg_used_present=np.zeros(1, np.uint8),
                    agg_min=np.zeros(8, np.int64), agg_min_present=np.zeros(1, np.uint8),
                    other_nominated=np.zeros(max(NS, 1) * 8, np.int64), other_nominated_present=np.zeros(max(NS, 1), np.uint8),
                    nom_ptr=np.zeros(NS + 1, np.int32), nom_priority=np.zeros(nn, np.int32), nom_pending_index=np.zeros(nn, np.int64),
                    nom_req=np.zeros(nn * 8, np.int64), nom_req_present=np.zeros(nn, np.uint8))
        fn = L.spx_flatten_quota
        self._ck_static(fn(pods.ref(), rc.ref() if rc else None, quota.ref(),
                           *[v.ctypes.data_as(t) for v, t in zip(cols.values(), fn.argtypes[3:])]))
        ns = dict(has_quota=quota.array("has_quota"), used=quota.array("used"), used_present=quota.array("used_present"),
                  max=quota.array("max"), max_present=quota.array("max_present"), min=quota.array("min"), min_present=quota.array("min_present"))
        return {"cols": cols, "ns": ns, "P": P, "NS": NS}

    _QUOTA_POD_COLS = ("pod_ns", "pod_priority", "pod_req", "pod_req_present")

    def upload_quota(self, f: dict, rows=None) -> None:
        cols = dict(f["cols"])
        P = f["P"] if rows is None else rows[1] - rows[0]
        cols.update(_rows({k: cols[k] for k in self._QUOTA_POD_COLS}, f["P"], rows))
        if rows is not None:  # a nominated pod is skipped when it is the pod under evaluation: indices are relative to this engine's rows
            cols["nom_pending_index"] = cols["nom_pending_index"] - rows[0]
        if P > 0:
            t = Table(self._hdr, "spx_quota_soa", n_pods=P, n_namespaces=f["NS"], **f["ns"], **cols)
            self._ck(self._lib.spx_upload_quota(self._h, t.ref()))
        self.n_pods = P

    def prefilter(self, plugin: int, row_begin: int = 0, row_end: Optional[int] = None) -> np.ndarray:
        row_end = self.n_pods if row_end is None else row_end
        out = np.zeros(row_end - row_begin, np.uint8)
        self._ck(self._lib.spx_fetch_prefilter(self._h, plugin, row_begin, row_end, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    # ------------------------------------------------------------------ CapacityScheduling.PostFilter: the preemption dry run
    _PREEMPT_NODE_COLS = ("present", "allocatable", "requested", "pod_ptr", "pod_priority", "pod_start", "pod_ns", "pod_fit_req", "pod_quota_req",
                          "pod_quota_req_present", "pod_flags", "pod_pdb_mask", "pod_hi_order", "nom_ptr", "nom_priority", "nom_fit_req", "nom_pending_row",
                          "pdb_ptr", "pdb_allowed")

    def flatten_preempt_nodes(self, nodes: Table, rc: Optional[Table], quota: Table, objects: Table) -> dict:
        """spx_node_objects + spx_preempt_objects -> the columns of spx_preempt_nodes_soa, plus "pod_src" (the table's pods as indices into
        the assigned-pod objects) and "N" (spx_flatten_preempt_nodes, called once to count and once to fill).  SpxError(SPX_ERR_ARG)
        names the node, or the assigned pod, the flattener refuses."""
        fn, N = self._lib.spx_flatten_preempt_nodes, int(nodes.struct.n_nodes)
        counts = [C.c_int64() for _ in range(4)]  # pods, nominated, PDB budgets, the refused node / pod
        head = [nodes.ref(), rc.ref() if rc else None, quota.ref(), objects.ref(), *map(C.byref, counts)]

        def call(arrays):
            rc_ = fn(*head, *arrays)
            if rc_ != 0:
                bad = int(counts[3].value)
                raise self._err(rc_, f"preempt flatten: refused at node {bad}" if bad >= 0 else f"preempt flatten: refused at assigned pod {-1 - bad}")

        call([None] * (len(fn.argtypes) - len(head)))
        A, M, B = (int(c.value) for c in counts[:3])
        i32, i64, u8, u32 = np.int32, np.int64, np.uint8, np.uint32
        cols = dict(present=np.zeros(N, u8), allocatable=np.zeros((N, 8), i64), requested=np.zeros((N, 8), i64), pod_ptr=np.zeros(N + 1, i32),
                    pod_src=np.zeros(A, i32), pod_priority=np.zeros(A, i32), pod_start=np.zeros(A, i64), pod_ns=np.zeros(A, i32),
                    pod_fit_req=np.zeros((A, 8), i64), pod_quota_req=np.zeros((A, 8), i64), pod_quota_req_present=np.zeros(A, u8), pod_flags=np.zeros(A, u8),
                    pod_pdb_mask=np.zeros(A, u32), pod_hi_order=np.zeros(A, i32), nom_ptr=np.zeros(N + 1, i32), nom_priority=np.zeros(M, i32),
                    nom_fit_req=np.zeros((M, 8), i64), nom_pending_row=np.zeros(M, i64), pdb_ptr=np.zeros(N + 1, i32), pdb_allowed=np.zeros(B, i32))
        keep = {k: (v if v.size else np.zeros(1, v.dtype)) for k, v in cols.items()}  # never hand C a NULL for an empty column
        call([keep[k].ctypes.data_as(t) for k, t in zip(cols, fn.argtypes[len(head):])])
        return {"N": N, **cols}

    def load_preempt_objects(self, t: dict) -> dict:
        """objects.build_preempt_tables' tables through the flatteners to the device: the quota tables, the node side and the pending pods'
        fit vectors (what computePodResourceRequest gives, as the NodeInfo charges it).  Returns flatten_preempt_nodes' columns."""
        fq = self.flatten_quota(t["pods"], t["rc"], t["quota"])
        self.upload_quota(fq)
        f = self.flatten_preempt_nodes(t["nodes"], t["rc"], t["quota"], t["preempt"])
        self.upload_preempt_nodes(f)
        self.upload_preempt_pods(fq["cols"]["pod_req"].reshape(-1, 8))
        f["nominated_quota"] = self.flatten_preempt_nominated_quota(t["nodes"], t["rc"], t["quota"], t["preempt"], len(f["nom_priority"]))
        self.upload_preempt_nominated_quota(f["nominated_quota"])
        return f

    def preempt_nodes_table(self, f: dict) -> Table:
        return Table(self._hdr, "spx_preempt_nodes_soa", n_nodes=f["N"], **{k: np.ascontiguousarray(f[k]) for k in self._PREEMPT_NODE_COLS})

    def preempt_check(self, f: dict) -> int:
        """the first node spx_upload_preempt_nodes would refuse (spx_preempt_check), -1 when the table is within the device's limits"""
        bad = C.c_int64(-1)
        rc = self._lib.spx_preempt_check(self.preempt_nodes_table(f).ref(), C.byref(bad))
        if rc != 0 and bad.value < 0:
            self._ck_static(rc)
        return int(bad.value)

    def upload_preempt_nodes(self, f: dict) -> None:
        """the node side of the dry run: flatten_preempt_nodes' columns (spx_upload_preempt_nodes); earlier results become stale"""
        self._ck(self._lib.spx_upload_preempt_nodes(self._h, self.preempt_nodes_table(f).ref()))
        self.n_nodes = f["N"]

    def upload_preempt_pods(self, fit_req) -> None:
        """fit_req [P][8]: what NodeResourcesFit reads of each pending pod (spx_upload_preempt_pods); earlier results become stale"""
        fit = np.ascontiguousarray(fit_req, dtype=np.int64).reshape(-1, 8)
        self._ck(self._lib.spx_upload_preempt_pods(self._h, Table(self._hdr, "spx_preempt_pods_soa", n_pods=len(fit), fit_req=fit).ref()))
        self.n_pods = len(fit)

    def _preempt_row_list(self, rows, node_mask, eligible=None, per_row=(), names="eligible"):
        """What the four preemption runs take per entry of `rows`, converted and checked: (len(rows), rows, eligible, node_mask) as C
        pointers, None staying NULL.  per_row: the caller's own columns, which like eligible must have one entry per row (`names`)."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        elig = None if eligible is None else np.ascontiguousarray(eligible, dtype=np.uint8)
        if any(len(v) != len(rows) for v in (*per_row, *(() if elig is None else (elig,)))):
            raise ValueError(f"{names} must have one entry per row")
        mask = None
        if node_mask is not None:
            mask = np.ascontiguousarray(node_mask, dtype=np.uint8)
            if mask.shape != (len(rows), self.n_nodes):
                raise ValueError("node_mask must be [len(rows)][n_nodes]")
        u8 = lambda v: None if v is None else v.ctypes.data_as(C.POINTER(C.c_uint8))  # (the pointer keeps its array alive)
        return len(rows), rows.ctypes.data_as(C.POINTER(C.c_int64)), u8(elig), u8(mask)

    def preempt_dry_run(self, rows, node_mask=None) -> None:
        """SelectVictimsOnNode for the pod rows `rows` x all nodes and the pick per row (spx_preempt_dry_run); node_mask [len(rows)][n_nodes],
        0 = excluded.  Asynchronous; the fetches below address a row by its index in `rows`."""
        n, rows_p, _, mask_p = self._preempt_row_list(rows, node_mask)
        self._ck(self._lib.spx_preempt_dry_run(self._h, rows_p, n, mask_p))
        self._preempt_rows = n

    _PREEMPT_NOMQ_COLS = ("ns", "quota_req", "quota_req_present")

    def flatten_preempt_nominated_quota(self, nodes: Table, rc: Optional[Table], quota: Table, objects: Table, n_nom: int) -> dict:
        """the nominated pods of spx_preempt_objects in the record order of flatten_preempt_nodes' table (n_nom of them) -> the columns of
        spx_preempt_nominated_quota_soa, plus "nom_src" (each record's index among the nominated-pod objects)
        (spx_flatten_preempt_nominated_quota, host only)"""
        out = {"nom_src": np.zeros(n_nom, np.int32), "ns": np.zeros(n_nom, np.int32), "quota_req": np.zeros((n_nom, 8), np.int64), "quota_req_present": np.zeros(n_nom, np.uint8)}
        keep = {k: (v if v.size else np.zeros(1, v.dtype)) for k, v in out.items()}  # never hand C a NULL for an empty column
        rc_ = self._lib.spx_flatten_preempt_nominated_quota(
            nodes.ref(), rc.ref() if rc else None, quota.ref(), objects.ref(), n_nom, keep["nom_src"].ctypes.data_as(C.POINTER(C.c_int32)),
            keep["ns"].ctypes.data_as(C.POINTER(C.c_int32)), keep["quota_req"].ctypes.data_as(C.POINTER(C.c_int64)), keep["quota_req_present"].ctypes.data_as(C.POINTER(C.c_uint8)))
        if rc_ != 0:
            raise self._err(rc_, f"preempt nominated flatten: refused (n_nom {n_nom} is not the node table's count, or a request it cannot hold)")
        return out

    def upload_preempt_nominated_quota(self, cols: dict) -> None:
        """flatten_preempt_nominated_quota's columns, one entry per nominated record of the uploaded node table
        (spx_upload_preempt_nominated_quota); earlier results become stale, and a later upload_preempt_nodes drops the table"""
        cols = {"ns": np.ascontiguousarray(cols["ns"], dtype=np.int32), "quota_req": np.ascontiguousarray(cols["quota_req"], dtype=np.int64).reshape(-1, 8),
                "quota_req_present": np.ascontiguousarray(cols["quota_req_present"], dtype=np.uint8)}
        self._ck(self._lib.spx_upload_preempt_nominated_quota(self._h, Table(self._hdr, "spx_preempt_nominated_quota_soa", n_nominated=len(cols["ns"]), **cols).ref()))

    def preempt_sequential(self, rows, eligible=None, node_mask=None) -> None:
        """CapacityScheduling's sequential preemption loop (spx_preempt_sequential): the rows are attempted once each in list order, each
        against the state the rows before it left (victims gone from their node and from their quota's Used, the preemptor nominated,
        lower nominations cleared, its own old nomination dropped).  eligible: per entry of rows, 0 = evaluated at its step but nothing
        applied (None = all).  The preempt_* fetches answer per row as it saw the state at its own step; preempt_victims answers for the
        row's picked node alone."""
        n, rows_p, elig_p, mask_p = self._preempt_row_list(rows, node_mask, eligible)
        self._ck(self._lib.spx_preempt_sequential(self._h, rows_p, n, elig_p, mask_p))
        self._preempt_rows = n

    def preempt_cells(self, i_begin: int = 0, i_end: Optional[int] = None):
        """(status uint8, n_victims, n_violations), each [i_end - i_begin][n_nodes] (spx_fetch_preempt_cells)"""
        i_end = getattr(self, "_preempt_rows", 0) if i_end is None else i_end
        n = max(i_end - i_begin, 0)
        st, nv, nx = np.zeros((n, self.n_nodes), np.uint8), np.zeros((n, self.n_nodes), np.int32), np.zeros((n, self.n_nodes), np.int32)
        i32 = C.POINTER(C.c_int32)
        self._ck(self._lib.spx_fetch_preempt_cells(self._h, i_begin, i_end, st.ctypes.data_as(C.POINTER(C.c_uint8)), nv.ctypes.data_as(i32), nx.ctypes.data_as(i32)))
        return st, nv, nx

    def preempt_keys(self, i_begin: int = 0, i_end: Optional[int] = None):
        """(highest victim priority int32, sum of priority + 2^31 int64, earliest start among the highest int64), each [rows][n_nodes]"""
        i_end = getattr(self, "_preempt_rows", 0) if i_end is None else i_end
        n = max(i_end - i_begin, 0)
        hi, sm, st = np.zeros((n, self.n_nodes), np.int32), np.zeros((n, self.n_nodes), np.int64), np.zeros((n, self.n_nodes), np.int64)
        i64 = C.POINTER(C.c_int64)
        self._ck(self._lib.spx_fetch_preempt_keys(self._h, i_begin, i_end, hi.ctypes.data_as(C.POINTER(C.c_int32)), sm.ctypes.data_as(i64), st.ctypes.data_as(i64)))
        return hi, sm, st

    def preempt_pick(self, i_begin: int = 0, i_end: Optional[int] = None) -> dict:
        """pickOneNodeForPreemption per row: node (-1 = none), n_victims, n_violations, n_candidates, n_ties (spx_fetch_preempt_pick)"""
        i_end = getattr(self, "_preempt_rows", 0) if i_end is None else i_end
        out = {k: np.zeros(max(i_end - i_begin, 0), np.int32) for k in ("node", "n_victims", "n_violations", "n_candidates", "n_ties")}
        self._ck(self._lib.spx_fetch_preempt_pick(self._h, i_begin, i_end, *[v.ctypes.data_as(C.POINTER(C.c_int32)) for v in out.values()]))
        return out

    def preempt_victims(self, i: int, node: int):
        """(status, victims as positions in the node's list, most important first) of one cell, recomputed (spx_fetch_preempt_victims)"""
        cap = self._hdr.consts["SPX_PREEMPT_MAX_NODE_PODS"]
        pos, n, st = np.zeros(cap, np.int32), C.c_int32(), C.c_int32()
        self._ck(self._lib.spx_fetch_preempt_victims(self._h, i, node, pos.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(n), C.byref(st)))
        return int(st.value), pos[:n.value].copy()

    def preempt_eligible(self, f: dict, quota: Table, over_min, ns, priority, preempt_never, nominated_node, nominated_unresolvable, more_than_min) -> np.ndarray:
        """PodEligibleToPreemptOthers per pod from the node table's terminating bits (spx_preempt_eligible, host only)"""
        u8, i32, i64 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        arr = lambda v, dt: np.ascontiguousarray(v, dtype=dt)
        om, ns, pr, never = arr(over_min, np.uint8), arr(ns, np.int32), arr(priority, np.int32), arr(preempt_never, np.uint8)
        nn, un, mm = arr(nominated_node, np.int64), arr(nominated_unresolvable, np.uint8), arr(more_than_min, np.uint8)
        out = np.zeros(len(ns), np.uint8)
        self._ck_static(self._lib.spx_preempt_eligible(self.preempt_nodes_table(f).ref(), quota.ref(), om.ctypes.data_as(u8), len(ns), ns.ctypes.data_as(i32),
                                                       pr.ctypes.data_as(i32), never.ctypes.data_as(u8), nn.ctypes.data_as(i64), un.ctypes.data_as(u8),
                                                       mm.ctypes.data_as(u8), out.ctypes.data_as(u8)))
        return out.astype(bool)

    # ------------------------------------------------------------------ PreemptionToleration.PostFilter: its dry run on the same tables
    _PTOL_COLS = ("min_preemptable", "exempt_until_ns", "flags")

    def flatten_preempt_toleration(self, classes: Table, pod_class, pod_scheduled, pod_scheduled_at_ns, pod_src) -> dict:
        """the PriorityClass table (objects.build_priority_classes) and, per assigned pod in object order, its class index (-1 = no name),
        whether it has a PodScheduled=True condition and since when -> the columns of spx_preempt_toleration_soa in the order of
        flatten_preempt_nodes' table, whose "pod_src" permutes them (spx_flatten_preempt_toleration, host only)"""
        arr = lambda v, dt: np.ascontiguousarray(v, dtype=dt)
        pc, sc, at, src = arr(pod_class, np.int32), arr(pod_scheduled, np.uint8), arr(pod_scheduled_at_ns, np.int64), arr(pod_src, np.int32)
        if not len(pc) == len(sc) == len(at):
            raise ValueError("the per-pod columns differ in length")
        A = len(src)
        out = {"min_preemptable": np.zeros(A, np.int32), "exempt_until_ns": np.zeros(A, np.int64), "flags": np.zeros(A, np.uint8)}
        ptr = lambda v, t: (v if v.size else np.zeros(1, v.dtype)).ctypes.data_as(C.POINTER(t))  # never hand C a NULL for an empty column
        self._ck_static(self._lib.spx_flatten_preempt_toleration(classes.ref(), len(pc), ptr(pc, C.c_int32), ptr(sc, C.c_uint8), ptr(at, C.c_int64), A, ptr(src, C.c_int32),
                                                                 out["min_preemptable"].ctypes.data_as(C.POINTER(C.c_int32)),
                                                                 out["exempt_until_ns"].ctypes.data_as(C.POINTER(C.c_int64)), out["flags"].ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def upload_preempt_toleration(self, cols: dict) -> None:
        """flatten_preempt_toleration's columns, one entry per pod of the uploaded node table (spx_upload_preempt_toleration); earlier
        results become stale, and a later upload_preempt_nodes drops the table"""
        n = len(cols["flags"])
        self._ck(self._lib.spx_upload_preempt_toleration(self._h, Table(self._hdr, "spx_preempt_toleration_soa", n_pods=n, **{k: cols[k] for k in self._PTOL_COLS}).ref()))

    def load_preempt_toleration_objects(self, t: dict) -> dict:
        """objects.build_preempt_toleration_tables' tables through the flatteners to the device: the node side, the pending pods' fit vectors
        and the toleration table.  No quota table is uploaded.  Returns flatten_preempt_nodes' columns plus "toleration"."""
        fq = self.flatten_quota(t["pods"], t["rc"], t["quota"])  # host only: computePodResourceRequest of the pending pods
        f = self.flatten_preempt_nodes(t["nodes"], t["rc"], t["quota"], t["preempt"])
        self.upload_preempt_nodes(f)
        self.upload_preempt_pods(fq["cols"]["pod_req"].reshape(-1, 8))
        f["toleration"] = self.flatten_preempt_toleration(t["classes"], t["pod_class"], t["pod_scheduled"], t["pod_scheduled_at_ns"], f["pod_src"])
        self.upload_preempt_toleration(f["toleration"])
        return f

    def preempt_toleration_dry_run(self, rows, priority, preempt_never, now_ns: int, node_mask=None) -> None:
        """PreemptionToleration's SelectVictimsOnNode for the pod rows `rows` x all nodes and the pick per row
        (spx_preempt_toleration_dry_run); priority / preempt_never per entry of rows, now_ns the plugin's clock.  The preempt_* fetches
        answer for this run until the next dry run of either kind."""
        prio, never = np.ascontiguousarray(priority, dtype=np.int32), np.ascontiguousarray(preempt_never, dtype=np.uint8)
        n, rows_p, _, mask_p = self._preempt_row_list(rows, node_mask, per_row=(prio, never), names="priority and preempt_never")
        self._ck(self._lib.spx_preempt_toleration_dry_run(self._h, rows_p, n, prio.ctypes.data_as(C.POINTER(C.c_int32)), never.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                          int(now_ns), mask_p))
        self._preempt_rows = n

    def preempt_toleration_sequential(self, rows, priority, preempt_never, now_ns: int, eligible=None, node_mask=None) -> None:
        """The sequential preemption loop (spx_preempt_toleration_sequential): the rows are attempted once each in list order, each against
        the state the rows before it left (victims gone, the preemptor nominated, lower nominations cleared, its own old nomination
        dropped).  eligible: per entry of rows, 0 = evaluated at its step but nothing applied (None = all).  The preempt_* fetches
        answer per row as it saw the state at its own step; preempt_victims answers for the row's picked node alone."""
        prio, never = np.ascontiguousarray(priority, dtype=np.int32), np.ascontiguousarray(preempt_never, dtype=np.uint8)
        n, rows_p, elig_p, mask_p = self._preempt_row_list(rows, node_mask, eligible, per_row=(prio, never), names="priority, preempt_never and eligible")
        self._ck(self._lib.spx_preempt_toleration_sequential(self._h, rows_p, n, prio.ctypes.data_as(C.POINTER(C.c_int32)), never.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                             elig_p, int(now_ns), mask_p))
        self._preempt_rows = n

    def preempt_toleration_eligible(self, f: dict, priority, preempt_never, nominated_node, nominated_unresolvable) -> np.ndarray:
        """PreemptionToleration's PodEligibleToPreemptOthers per pod (spx_preempt_toleration_eligible, host only)"""
        u8, i32, i64 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        arr = lambda v, dt: np.ascontiguousarray(v, dtype=dt)
        pr, never, nn, un = arr(priority, np.int32), arr(preempt_never, np.uint8), arr(nominated_node, np.int64), arr(nominated_unresolvable, np.uint8)
        out = np.zeros(len(pr), np.uint8)
        self._ck_static(self._lib.spx_preempt_toleration_eligible(self.preempt_nodes_table(f).ref(), len(pr), pr.ctypes.data_as(i32), never.ctypes.data_as(u8),
                                                                  nn.ctypes.data_as(i64), un.ctypes.data_as(u8), out.ctypes.data_as(u8)))
        return out.astype(bool)

    # ------------------------------------------------------------------ the toleration dry run with NRT's single-NUMA Filter in the refit
    _PNRT_NODE_COLS = ("node_flags", "n_zones", "zone_id", "zone_present", "node_present", "zone_avail", "zone_headroom")
    _PNRT_POD_COLS = ("pod_contributes", "rel_ptr", "rel_zone", "rel_slot", "rel_qty")

    def flatten_preempt_nrt(self, nodes: Table, nrt: Table, rc: Optional[Table], pods: Table, objects: Table, pod_src, ctr_numa, placement_present,
                            placement_containers, params: Optional[Table] = None) -> dict:
        """the NRT side table of the preemption tables (spx_flatten_nrt_slots, spx_flatten_preempt_nrt, spx_flatten_nrt_pods; host only):
        `pods` the pending batch, `objects` the spx_preempt_objects of flatten_preempt_nodes and pod_src its column; ctr_numa per container
        of the assigned pods (NUMA id, -1, SPX_EVICT_CTR_UNKNOWN), placement_present / placement_containers per node.  Returns "slots",
        "R", the node and assigned-pod columns of spx_preempt_nrt_soa and "pods" (the preemptors' records).  SpxError(SPX_ERR_ARG) names
        the node or the assigned pod the flattener refuses."""
        L, H = self._lib, self._hdr
        u8p, i32p, i64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        n_res, slot_res, slot_flags, slot_weight = C.c_int32(), np.zeros(8, np.int32), np.zeros(8, np.uint8), np.zeros(8, np.int64)
        rc_p = rc.ref() if rc else None
        rc_ = L.spx_flatten_nrt_slots(pods.ref(), nrt.ref(), rc_p, params.ref() if params else None, C.byref(n_res), slot_res.ctypes.data_as(i32p),
                                      slot_flags.ctypes.data_as(u8p), slot_weight.ctypes.data_as(i64p))
        if rc_ != 0:
            raise self._err(rc_, "preempt nrt flatten: more than SPX_NRT_MAX_RES resource slots (the wide tables are not taken here)")
        R = n_res.value
        slots = Table(H, "spx_nrt_slots", n_res=R, slot_res=slot_res, slot_flags=slot_flags, slot_weight=slot_weight)
        arr = lambda v, dt: np.ascontiguousarray(v, dtype=dt)
        src, numa, pp, pcnt = arr(pod_src, np.int32), arr(ctr_numa, np.int32), arr(placement_present, np.uint8), arr(placement_containers, np.int32)
        N, A = int(nodes.struct.n_nodes), len(src)
        if len(pp) != N or len(pcnt) != N:
            raise ValueError("placement_present / placement_containers must have one entry per node")
        cols = dict(node_flags=np.zeros(N, np.uint8), n_zones=np.zeros(N, np.uint8), zone_id=np.zeros((N, 8), np.uint8), zone_present=np.zeros((N, 8), np.uint8),
                    node_present=np.zeros(N, np.uint8), zone_avail=np.zeros((N, 8, max(R, 1)), np.int64), zone_headroom=np.zeros((N, 8, max(R, 1)), np.int64),
                    pod_contributes=np.zeros(A, np.uint8), rel_ptr=np.zeros(A + 1, np.int32))
        ptr = lambda v, t: (v if v.size else np.zeros(1, v.dtype)).ctypes.data_as(t)  # never hand C a NULL for an empty column
        n_rel, bad, cap = C.c_int64(), C.c_int64(), 64
        while True:
            rel = dict(rel_zone=np.zeros(cap, np.uint8), rel_slot=np.zeros(cap, np.uint8), rel_qty=np.zeros(cap, np.int64))
            rc_ = L.spx_flatten_preempt_nrt(nodes.ref(), nrt.ref(), rc_p, slots.ref(), objects.ref(), ptr(numa, i32p), ptr(pp, u8p), ptr(pcnt, i32p), A, ptr(src, i32p), cap,
                                            C.byref(n_rel), C.byref(bad), *[ptr(cols[k], t) for k, t in zip(cols, (u8p, u8p, u8p, u8p, u8p, i64p, i64p, u8p, i32p))],
                                            rel["rel_zone"].ctypes.data_as(u8p), rel["rel_slot"].ctypes.data_as(u8p), rel["rel_qty"].ctypes.data_as(i64p))
            if rc_ == 0 or n_rel.value <= cap:
                break
            cap = int(n_rel.value)
        if rc_ != 0:
            b = int(bad.value)
            what = f"node {b}" if b >= 0 else f"assigned pod {-1 - b}" if b > -(1 << 63) else "its arguments"
            raise self._err(rc_, f"preempt nrt flatten: refused at {what}")
        cols.update({k: v[:n_rel.value] for k, v in rel.items()})
        return {"slots": slots, "R": R, "N": N, **cols, "pods": self.flatten_nrt_pods(pods, rc, slots)}

    def preempt_nrt_table(self, f: dict) -> Table:
        pc = f["pods"]
        pods = Table(self._hdr, "spx_nrt_pods_soa", n_pods=len(pc["qos"]), n_res=f["R"], **{k: pc[k] for k in pc})
        return Table(self._hdr, "spx_preempt_nrt_soa", n_nodes=f["N"], slots=f["slots"], n_assigned=len(f["pod_contributes"]), pods=pods,
                     **{k: f[k] for k in self._PNRT_NODE_COLS + self._PNRT_POD_COLS})

    def preempt_nrt_check(self, f: dict):
        """(kind, index) of spx_flatten_preempt_nrt_check: (0, -1) when the table is within the device's limits, else what it names"""
        kind, bad = C.c_int32(), C.c_int64()
        self._lib.spx_flatten_preempt_nrt_check(self.preempt_nrt_table(f).ref(), C.byref(kind), C.byref(bad))
        return int(kind.value), int(bad.value)

    def upload_preempt_nrt(self, f: dict) -> None:
        """flatten_preempt_nrt's table, for the node and pod tables in place (spx_upload_preempt_nrt); earlier results become stale, and a
        later upload_preempt_nodes or upload_preempt_pods drops the table"""
        self._ck(self._lib.spx_upload_preempt_nrt(self._h, self.preempt_nrt_table(f).ref()))

    def preempt_toleration_nrt_dry_run(self, rows, priority, preempt_never, now_ns: int, node_mask=None, preemption_mode: bool = True) -> None:
        """preempt_toleration_dry_run with NodeResourceTopologyMatch's Filter in the refit (spx_preempt_toleration_nrt_dry_run): the
        Filter sees the pods removed so far as its preemption stack; preemption_mode False: it never does, and is the ordinary Filter.
        The preempt_* fetches answer for this run until the next dry run of any kind."""
        prio, never = np.ascontiguousarray(priority, dtype=np.int32), np.ascontiguousarray(preempt_never, dtype=np.uint8)
        n, rows_p, _, mask_p = self._preempt_row_list(rows, node_mask, per_row=(prio, never), names="priority and preempt_never")
        self._ck(self._lib.spx_preempt_toleration_nrt_dry_run(self._h, rows_p, n, prio.ctypes.data_as(C.POINTER(C.c_int32)), never.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                              int(now_ns), mask_p, 1 if preemption_mode else 0))
        self._preempt_rows = n

    def preempt_toleration_nrt_sequential(self, rows, priority, preempt_never, now_ns: int, eligible=None, node_mask=None, preemption_mode: bool = True) -> None:
        """preempt_toleration_sequential with NodeResourceTopologyMatch's Filter in the refit (spx_preempt_toleration_nrt_sequential), on
        upload_preempt_nrt's side table, which stays as uploaded at every step: a pod evicted at an earlier step is never on the Filter's
        stack again.  preemption_mode False: the ordinary Filter at every step.  The preempt_* fetches answer as after
        preempt_toleration_sequential."""
        prio, never = np.ascontiguousarray(priority, dtype=np.int32), np.ascontiguousarray(preempt_never, dtype=np.uint8)
        n, rows_p, elig_p, mask_p = self._preempt_row_list(rows, node_mask, eligible, per_row=(prio, never), names="priority, preempt_never and eligible")
        self._ck(self._lib.spx_preempt_toleration_nrt_sequential(self._h, rows_p, n, prio.ctypes.data_as(C.POINTER(C.c_int32)), never.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                                 elig_p, int(now_ns), mask_p, 1 if preemption_mode else 0))
        self._preempt_rows = n

    def preempt_nrt_dry_run(self, rows, node_mask=None, preemption_mode: bool = True) -> None:
        """preempt_dry_run with NodeResourceTopologyMatch's Filter in the refit (spx_preempt_nrt_dry_run), on the quota and preemption
        tables and upload_preempt_nrt's side table: the Filter sees the pods removed so far, those taken for the quota included, as its
        preemption stack; preemption_mode False: it never does, and is the ordinary Filter.  The preempt_* fetches answer for this run
        until the next dry run of any kind."""
        n, rows_p, _, mask_p = self._preempt_row_list(rows, node_mask)
        self._ck(self._lib.spx_preempt_nrt_dry_run(self._h, rows_p, n, mask_p, 1 if preemption_mode else 0))
        self._preempt_rows = n

    def preempt_nrt_sequential(self, rows, eligible=None, node_mask=None, preemption_mode: bool = True) -> None:
        """preempt_sequential with NodeResourceTopologyMatch's Filter in the refit (spx_preempt_nrt_sequential), on the quota and
        preemption tables, the nominated-quota side table and upload_preempt_nrt's side table, which stays as uploaded at every step: a
        pod evicted at an earlier step is never on the Filter's stack again, and a victim the Filter alone kept leaves its quota's Used
        like any other.  preemption_mode False: the ordinary Filter at every step.  The preempt_* fetches answer as after
        preempt_sequential."""
        n, rows_p, elig_p, mask_p = self._preempt_row_list(rows, node_mask, eligible)
        self._ck(self._lib.spx_preempt_nrt_sequential(self._h, rows_p, n, elig_p, mask_p, 1 if preemption_mode else 0))
        self._preempt_rows = n

    def status(self, plugin: int, pod_row: int) -> np.ndarray:
        out = np.empty(self.n_nodes, dtype=np.uint8)
        self._ck(self._lib.spx_fetch_status(self._h, plugin, pod_row, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def all_status(self, plugin: int, row_begin: int = 0, row_end: Optional[int] = None) -> np.ndarray:
        """[rows][n_nodes] uint8 in one strided copy (spx_fetch_status_rows)"""
        row_end = self.n_pods if row_end is None else row_end
        out = np.empty((row_end - row_begin, self.n_nodes), dtype=np.uint8)
        self._ck(self._lib.spx_fetch_status_rows(self._h, plugin, row_begin, row_end, out.ctypes.data_as(C.POINTER(C.c_uint8)), self.n_nodes))
        return out

    # ------------------------------------------------------------------ eval / fetch
    def eval(self, plugin_mask: int, row_begin: int = 0, row_end: Optional[int] = None) -> None:
        self._ck(self._lib.spx_eval(self._h, plugin_mask, row_begin, self.n_pods if row_end is None else row_end))

    def sync(self) -> None:
        self._ck(self._lib.spx_sync(self._h))

    def kernel_path(self, plugin: int) -> int:
        """0 = generic sweep kernel, 1 = fast formulation (same results); NETOVERHEAD: 2 = the 64-bit sweep (costs that need int64)."""
        return int(self._lib.spx_kernel_path(self._h, plugin))

    # ------------------------------------------------------------------ one-call loaders (spx_load_*: flatten + upload inside the library)
    def load_c(self, snap: dict, nrt_params: Optional[Table] = None, concurrent: bool = False) -> None:
        """the object tables of `snap` (keys as synth.full_snapshot's) through spx_load_trimaran / _nrt / _network / _quota — the calls
        the cgo shim makes — instead of this module's own flatten_* + upload_* sequences"""
        L = self._lib
        ref = lambda t: t.ref() if t is not None else None
        if concurrent:  # spx_load_profile: the four loaders side by side inside the library
            keys = {"nodes": "nodes", "rc": "rc", "pods": "pods", "metrics": "metrics", "assigned": "assigned", "nrt": "nrt", "appgroups": "appgroups",
                    "nettopo": "nettopo", "quota": "quota"}
            fields = {k: snap[v] for k, v in keys.items() if snap.get(v) is not None}
            if "nrt" in fields:
                fields["nrt_params"] = nrt_params
            self._ck(L.spx_load_profile(self._h, Table(self._hdr, "spx_profile_objects", **fields).ref()))
            self.n_pods = snap["pods"].struct.n_pods
            self.n_nodes = snap["nodes"].struct.n_nodes
            return
        if "metrics" in snap:
            self._ck(L.spx_load_trimaran(self._h, snap["nodes"].ref(), ref(snap.get("rc")), snap["pods"].ref(), snap["metrics"].ref(), ref(snap.get("assigned"))))
        if "nrt" in snap:
            self._ck(L.spx_load_nrt(self._h, snap["nodes"].ref(), snap["nrt"].ref(), ref(snap.get("rc")), snap["pods"].ref(), nrt_params.ref()))
        if "appgroups" in snap:
            self._ck(L.spx_load_network(self._h, snap["nodes"].ref(), snap["pods"].ref(), snap["appgroups"].ref(), snap["nettopo"].ref()))
        if "quota" in snap:
            self._ck(L.spx_load_quota(self._h, snap["pods"].ref(), ref(snap.get("rc")), snap["quota"].ref()))
        self.n_pods = snap["pods"].struct.n_pods
        if "nodes" in snap:
            self.n_nodes = snap["nodes"].struct.n_nodes

    def last_load_nrt_ms(self) -> Dict[str, float]:
        """wall time of the stages of the last spx_load_nrt (spx_last_load_nrt_ms)"""
        ms = (C.c_double * 6)()
        self._ck(self._lib.spx_last_load_nrt_ms(self._h, ms))
        return dict(zip(("flatten_slots", "flatten_nodes", "flatten_pods", "params_slot_table", "upload_nodes", "upload_pods"), (float(x) for x in ms)))

    def load_trimaran_pods(self, pods: Table) -> None:
        """a new pending batch for Allocatable / TLP / LVRB: flattened straight into the engine's pinned staging (spx_load_trimaran_pods)"""
        self._ck(self._lib.spx_load_trimaran_pods(self._h, pods.ref()))
        self.n_pods = pods.struct.n_pods

    def nrt_packed_score_slots(self):
        """None when LeastAllocated's Score launch keeps float64; else (mask of the weighted NRT slots scored in packed float32
        unconditionally, the slot scored that way through the per-launch table or -1) — spx_nrt_packed_score_slots"""
        v = int(self._lib.spx_nrt_packed_score_slots(self._h))
        if v < 0:
            self._ck(v)
        if v == 0:
            return None
        return v & 0xffff, ((v >> 16) & 0xff) - 1

    def nrt_filter_path(self) -> int:
        """which Filter launch the last NRT sweep ran: 1 float64 compares, 2 rank space"""
        return int(self._lib.spx_nrt_filter_path(self._h))

    def commit_path(self) -> int:
        """which form the last commit_sequential ran: 1 one-workgroup trimaran chain, 2 per-pod launches, 3 cooperative kernel"""
        return int(self._lib.spx_commit_path(self._h))

    def last_eval_ms(self) -> float:
        ms = C.c_float()
        self._ck(self._lib.spx_last_eval_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def scores(self, plugin: int, pod_row: int) -> np.ndarray:
        out = np.empty(self.n_nodes, dtype=np.uint8)
        self._ck(self._lib.spx_fetch_scores(self._h, plugin, pod_row, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def raw(self, plugin: int, pod_row: int, which: int = 0) -> np.ndarray:
        out = np.empty(self.n_nodes, dtype=np.int64)
        self._ck(self._lib.spx_fetch_raw(self._h, plugin, which, pod_row, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def score_table(self, plugin: int):
        """(device pointer, row stride in bytes, rows) of a plugin's uint8 table in HBM."""
        p = C.c_void_p()
        stride = C.c_int64()
        rows = C.c_int64()
        self._ck(self._lib.spx_score_table(self._h, plugin, C.byref(p), C.byref(stride), C.byref(rows)))
        return p.value, stride.value, rows.value

    def bind_score_table(self, plugin: int, dptr: int, row_stride: int, n_rows: int) -> None:
        self._ck(self._lib.spx_bind_score_table(self._h, plugin, C.c_void_p(dptr), row_stride, n_rows))

    def bind_status_table(self, plugin: int, dptr: int, row_stride: int, n_rows: int) -> None:
        """a Filter plugin's (NRT, NETOVERHEAD) uint8 status table in caller-owned memory, rows of the engine row stride; dptr 0 unbinds"""
        self._ck(self._lib.spx_bind_status_table(self._h, plugin, C.c_void_p(dptr), row_stride, n_rows))

    def upload_feasible_mask(self, mask: Optional[np.ndarray]) -> None:
        """[n_pods][n_nodes] uint8, non-zero = the node passed the caller's other Filter plugins; None clears it."""
        if mask is None:
            self._ck(self._lib.spx_upload_feasible_mask(self._h, None, 0, 0))
            return
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        self._ck(self._lib.spx_upload_feasible_mask(self._h, mask.ctypes.data_as(C.POINTER(C.c_uint8)), mask.shape[0], mask.shape[1]))
        self.n_pods, self.n_nodes = mask.shape  # (the upload fixes the engine's shape when no table has)

    def set_plugin_weights(self, weights: Dict[int, int]) -> None:
        w = np.ones(NUM_PLUGINS, dtype=np.int64)
        for k, v in weights.items():
            w[k] = v
        self._ck(self._lib.spx_set_plugin_weights(self._h, w.ctypes.data_as(C.POINTER(C.c_int64))))

    def eval_best(self, plugin_mask: int, row_begin: int = 0, row_end: Optional[int] = None) -> None:
        self._ck(self._lib.spx_eval_best(self._h, plugin_mask, row_begin, self.n_pods if row_end is None else row_end))

    def decide(self, plugin_mask: int, row_begin: int = 0, row_end: Optional[int] = None) -> None:
        """eval + per-row argmax without materialising score tables where the profile allows (spx_decide); read with best()"""
        self._ck(self._lib.spx_decide(self._h, plugin_mask, row_begin, self.n_pods if row_end is None else row_end))

    def best(self, row_begin: int = 0, row_end: Optional[int] = None):
        """(best node, weighted score, ties, feasible count) per pod row."""
        row_end = self.n_pods if row_end is None else row_end
        n = row_end - row_begin
        node, score = np.zeros(n, np.int32), np.zeros(n, np.int64)
        ties, feas = np.zeros(n, np.int32), np.zeros(n, np.int32)
        i32p = C.POINTER(C.c_int32)
        self._ck(self._lib.spx_fetch_best(self._h, row_begin, row_end, node.ctypes.data_as(i32p), score.ctypes.data_as(C.POINTER(C.c_int64)),
                                          ties.ctypes.data_as(i32p), feas.ctypes.data_as(i32p)))
        return node, score, ties, feas

    def commit_sequential(self, plugin_mask: int, row_begin: int = 0, row_end: Optional[int] = None, want_ties: bool = True):
        """pods in row order, each seeing the commits before it -> (node, weighted score, ties, missing); plugin_mask may hold
        Allocatable / TLP / LVRB / NRT / NetworkOverhead / CapacityScheduling / LowRiskOverCommitment / Peaks (spx_commit_sequential;
        the last two with their tables loaded: a bound pod joins its node's LROC sums, Peaks is normalised per pod over the pod's
        feasible nodes); SySched, NodeMetadata and PodState are rejected"""
        row_end = self.n_pods if row_end is None else row_end
        n = row_end - row_begin
        node, score, ties = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int32)
        missing = np.zeros(self.n_nodes, np.int64)
        self._ck(self._lib.spx_commit_sequential(self._h, plugin_mask, row_begin, row_end, node.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 score.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 ties.ctypes.data_as(C.POINTER(C.c_int32)) if want_ties else None,
                                                 missing.ctypes.data_as(C.POINTER(C.c_int64))))
        return node, score, (ties if want_ties else None), missing

    def set_stream(self, stream: int) -> None:
        self._ck(self._lib.spx_set_stream(self._h, C.c_void_p(stream)))

    def all_scores(self, plugin: int, row_begin: int = 0, row_end: Optional[int] = None) -> np.ndarray:
        """[rows][n_nodes] uint8 in one strided copy (spx_fetch_score_rows)"""
        row_end = self.n_pods if row_end is None else row_end
        out = np.empty((row_end - row_begin, self.n_nodes), dtype=np.uint8)
        self._ck(self._lib.spx_fetch_score_rows(self._h, plugin, row_begin, row_end, out.ctypes.data_as(C.POINTER(C.c_uint8)), self.n_nodes))
        return out
