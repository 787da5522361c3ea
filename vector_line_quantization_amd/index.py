"""Python handle over the C ABI.  Arguments may be numpy arrays (host) or torch
tensors (host or device: only .data_ptr() is taken -- torch is plumbing for device
memory and streams, never compute).  The library issues its work on the index's own stream:
hand over device tensors only after the stream that produced them has finished, or make the
index use that stream (`set_stream(torch.cuda.current_stream().cuda_stream)`)."""
import ctypes as C

import numpy as np

from ._lib import check, lib


def _is_torch(a):
    return hasattr(a, "data_ptr") and hasattr(a, "is_contiguous")


def _ptr(a, np_dtype=None):
    """(pointer, keepalive) of a numpy array or torch tensor; None -> NULL."""
    if a is None:
        return None, None
    if _is_torch(a):
        if not a.is_contiguous():
            a = a.contiguous()
        return C.c_void_p(a.data_ptr()), a
    a = np.ascontiguousarray(a, dtype=np_dtype)
    return a.ctypes.data_as(C.c_void_p), a


def _out_ptr(a, np_dtype):
    """Pointer of an OUTPUT buffer: it must be written in place, so a buffer that would need a
    contiguous (or dtype-converted) copy is an error, never a silent temporary."""
    if _is_torch(a):
        if not a.is_contiguous():
            raise ValueError("output tensor must be contiguous (the library writes it in place)")
        want = {np.float32: "torch.float32", np.int64: "torch.int64"}.get(np_dtype)
        if want is not None and str(a.dtype) != want:
            raise ValueError("output tensor must be %s, got %s" % (want, a.dtype))
        return C.c_void_p(a.data_ptr()), a
    if not isinstance(a, np.ndarray) or not a.flags["C_CONTIGUOUS"] or a.dtype != np.dtype(np_dtype) or not a.flags["WRITEABLE"]:
        raise ValueError("output array must be a writeable C-contiguous numpy array of dtype %s" % np.dtype(np_dtype).name)
    return a.ctypes.data_as(C.c_void_p), a


class GpuIVFPQ:
    """Mirror of the data-carrying surface of faiss::gpu::GpuIndexIVFPQ
    (gpu/GpuIndexIVFPQ.h:41-234) / faiss::IndexIVFPQ (IndexIVFPQ.h:29-164) for the
    search path: construct, copy trained state in, search."""

    METRICS = {"ip": 0, "l2": 1}      # the reference's MetricType (Index.h)

    def __init__(self, d, nlist, M, nbits, device=0, metric="l2"):
        self.d, self.nlist, self.M, self.nbits = d, nlist, M, nbits
        self.ksub = 1 << nbits
        self._h = C.c_void_p()
        if metric not in self.METRICS:
            raise ValueError("metric %r (one of 'l2', 'ip')" % (metric,))
        check(lib().vlq_ivfpq_create(C.byref(self._h), C.c_int(device), C.c_int(d), C.c_int(nlist),
                                     C.c_int(M), C.c_int(nbits)))
        self.device = device
        if metric != "l2":
            self.metric = metric

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().vlq_ivfpq_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- state ------------------------------------------------------------
    def set_stream(self, stream_ptr):
        check(lib().vlq_ivfpq_set_stream(self._h, C.c_void_p(stream_ptr or 0)))

    def set_coarse_centroids(self, c):
        p, _k = _ptr(c, np.float32)
        check(lib().vlq_ivfpq_set_coarse_centroids(self._h, p))

    def set_imi_centroids(self, imi_nbits, c):
        p, _k = _ptr(c, np.float32)
        check(lib().vlq_ivfpq_set_imi_centroids(self._h, C.c_int(imi_nbits), p))

    def set_pq_centroids(self, c):
        p, _k = _ptr(c, np.float32)
        check(lib().vlq_ivfpq_set_pq_centroids(self._h, p))

    def set_search_options(self, by_residual=True, use_precomputed_table=1, max_codes=0):
        check(lib().vlq_ivfpq_set_search_options(self._h, C.c_int(int(by_residual)),
                                                 C.c_int(use_precomputed_table), C.c_int64(max_codes)))

    @property
    def metric(self):
        """"l2" (ascending squared distances) or "ip" (IndexIVFPQ with METRIC_INNER_PRODUCT: descending inner products,
        -FLT_MAX / -1 padding; include/vlq_ivfpq.h says what is served)"""
        m = C.c_int(1)
        check(lib().vlq_ivfpq_get_metric(self._h, C.byref(m)))
        return "ip" if m.value == 0 else "l2"

    @metric.setter
    def metric(self, metric):
        if metric not in self.METRICS:
            raise ValueError("metric %r (one of 'l2', 'ip')" % (metric,))
        check(lib().vlq_ivfpq_set_metric(self._h, C.c_int(self.METRICS[metric])))

    def set_float16_tables(self, enable=True):
        """GpuIndexIVFPQConfig::useFloat16LookupTables for the plain IVFPQ search (include/vlq_ivfpq.h)"""
        check(lib().vlq_ivfpq_set_float16_tables(self._h, C.c_int(int(enable))))

    def set_coarse_screen(self, mode):
        """0 off, 1 on (default): float16 screen in front of the exact coarse distances (speed only; include/vlq_ivfpq.h)"""
        check(lib().vlq_ivfpq_set_coarse_screen(self._h, C.c_int(int(mode))))

    def coarse_screen_state(self):
        """(enabled, rows screened so far, rows the screen handed to the exact path)"""
        en, rows, und = C.c_int(0), C.c_uint64(0), C.c_uint32(0)
        check(lib().vlq_ivfpq_coarse_screen_state(self._h, C.byref(en), C.byref(rows), C.byref(und)))
        return bool(en.value), int(rows.value), int(und.value)

    def set_scan_sums(self, mode):
        """0 stored rows, 1 automatic (default): stored table sums in the 16-byte scan (speed and memory only; include/vlq_ivfpq.h)"""
        check(lib().vlq_ivfpq_set_scan_sums(self._h, C.c_int(int(mode))))

    def scan_sums_state(self):
        """(enabled, queries scanned on sums, queries redone on stored rows, codes redone exactly)"""
        en, seen, und, fin = C.c_int(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(lib().vlq_ivfpq_scan_sums_state(self._h, C.byref(en), C.byref(seen), C.byref(und), C.byref(fin)))
        return bool(en.value), int(seen.value), int(und.value), int(fin.value)

    def set_scan_schedule(self, mode):
        """0 automatic, 1 query-major, 2 list-owned (speed only; include/vlq_ivfpq.h)"""
        check(lib().vlq_ivfpq_set_scan_schedule(self._h, C.c_int(int(mode))))

    def set_polysemous_ht(self, ht):
        """IndexIVFPQ::polysemous_ht: 0 off; > 0 only codes within that Hamming distance of the query's code are looked up
        (include/vlq_ivfpq.h says which code that is in every mode)"""
        check(lib().vlq_ivfpq_set_polysemous_ht(self._h, C.c_int(int(ht))))
        self._polysemous_ht = int(ht)

    @property
    def polysemous_ht(self):
        return getattr(self, "_polysemous_ht", 0)

    @polysemous_ht.setter
    def polysemous_ht(self, ht):
        self.set_polysemous_ht(ht)

    def set_lists(self, codes, ids, list_offsets):
        pc, _a = _ptr(codes, np.uint8)
        pi, _b = _ptr(ids, np.int64)
        po, _c = _ptr(list_offsets, np.int64)
        check(lib().vlq_ivfpq_set_lists(self._h, pc, pi, po))

    @property
    def ntotal(self):
        return int(lib().vlq_ivfpq_ntotal(self._h))

    def list_length(self, i):
        n = C.c_int64()
        check(lib().vlq_ivfpq_list_length(self._h, C.c_int(i), C.byref(n)))
        return n.value

    def get_list(self, i):
        n = self.list_length(i)
        codes = np.empty((n, self.M), np.uint8)
        ids = np.empty((n,), np.int64)
        check(lib().vlq_ivfpq_get_list(self._h, C.c_int(i), codes.ctypes.data_as(C.c_void_p),
                                       ids.ctypes.data_as(C.c_void_p)))
        return codes, ids

    # --- add --------------------------------------------------------------
    def add(self, x, xids=None):
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        pi, _b = _ptr(xids, np.int64)
        check(lib().vlq_ivfpq_add(self._h, C.c_int64(n), px, pi))

    def reserve_memory(self, num_vecs):
        """GpuIndexIVFPQ::reserveMemory: room for num_vecs / nlist vectors in every list."""
        check(lib().vlq_ivfpq_reserve_memory(self._h, C.c_int64(num_vecs)))

    def reclaim_memory(self):
        """GpuIndexIVFPQ::reclaimMemory: drop the append slack; returns the device bytes freed."""
        n = C.c_uint64()
        check(lib().vlq_ivfpq_reclaim_memory(self._h, C.byref(n)))
        return n.value

    def encode(self, x):
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        assign = np.empty((n,), np.int64)
        codes = np.empty((n, self.M), np.uint8)
        check(lib().vlq_ivfpq_encode(self._h, C.c_int64(n), px, assign.ctypes.data_as(C.c_void_p),
                                     codes.ctypes.data_as(C.c_void_p)))
        return assign, codes

    # --- search -----------------------------------------------------------
    def encode_preassigned(self, x, assign):
        """codes of x for the given lists (IndexIVFPQ::encode_multiple, compute_keys = false)"""
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        pa, _b = _ptr(assign, np.int64)
        codes = np.empty((n, self.M), np.uint8)
        check(lib().vlq_ivfpq_encode_preassigned(self._h, C.c_int64(n), px, pa, codes.ctypes.data_as(C.c_void_p)))
        return codes

    def _out(self, out, shape, dtype, like):
        if out is not None:
            return out
        if _is_torch(like) and like.is_cuda:
            import torch
            return torch.empty(shape, dtype={np.float32: torch.float32, np.int64: torch.int64}[dtype],
                               device=like.device)
        return np.empty(shape, dtype)

    def search(self, x, nprobe, k, D=None, I=None):
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        D = self._out(D, (n, k), np.float32, x)
        I = self._out(I, (n, k), np.int64, x)
        pD, _b = _out_ptr(D, np.float32)
        pI, _c = _out_ptr(I, np.int64)
        check(lib().vlq_ivfpq_search(self._h, C.c_int64(n), px, C.c_int(nprobe), C.c_int(k), pD, pI))
        return D, I

    def search_preassigned(self, x, keys, coarse_dis, k, store_pairs=False, D=None, I=None):
        n = x.shape[0]
        nprobe = keys.shape[1]
        px, _a = _ptr(x, np.float32)
        pk, _b = _ptr(keys, np.int64)
        pc, _c = _ptr(coarse_dis, np.float32)
        D = self._out(D, (n, k), np.float32, x)
        I = self._out(I, (n, k), np.int64, x)
        pD, _d = _out_ptr(D, np.float32)
        pI, _e = _out_ptr(I, np.int64)
        check(lib().vlq_ivfpq_search_preassigned(self._h, C.c_int64(n), px, pk, pc, C.c_int(nprobe),
                                                 C.c_int(k), pD, pI, C.c_int(int(store_pairs))))
        return D, I

    def coarse_search(self, x, nprobe, cdis=None, keys=None):
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        cdis = self._out(cdis, (n, nprobe), np.float32, x)
        keys = self._out(keys, (n, nprobe), np.int64, x)
        pc, _b = _out_ptr(cdis, np.float32)
        pk, _c = _out_ptr(keys, np.int64)
        check(lib().vlq_ivfpq_coarse_search(self._h, C.c_int64(n), px, C.c_int(nprobe), pc, pk))
        return cdis, keys

    # --- IVFPQR: the re-ranking stage (IndexIVFPQ.h:200-225) -----------------
    def set_refine_pq(self, M_refine, nbits_refine, centroids):
        """IndexIVFPQR::refine_pq: centroids [M_refine][2^nbits_refine][d / M_refine]"""
        p, _k = _ptr(centroids, np.float32)
        check(lib().vlq_ivfpq_set_refine_pq(self._h, C.c_int(M_refine), C.c_int(nbits_refine), p))
        self.M_refine, self.nbits_refine = M_refine, nbits_refine

    def set_refine_codes(self, refine_codes):
        """refine codes [ntotal][M_refine] in the list-contiguous order of set_lists' codes (by list slot, not by id)"""
        p, _k = _ptr(refine_codes, np.uint8)
        check(lib().vlq_ivfpq_set_refine_codes(self._h, p))

    def get_list_refine_codes(self, i):
        out = np.empty((self.list_length(i), getattr(self, "M_refine", 0)), np.uint8)
        check(lib().vlq_ivfpq_get_list_refine_codes(self._h, C.c_int(i), out.ctypes.data_as(C.c_void_p)))
        return out

    def refine(self, x, shortlist, k, D=None, I=None):
        """the loop of IndexIVFPQR::search alone: shortlist [n][k_coarse] of list << 32 | offset labels (-1 = skip)"""
        n, k_coarse = x.shape[0], shortlist.shape[1]
        px, _a = _ptr(x, np.float32)
        ps, _b = _ptr(shortlist, np.int64)
        D = self._out(D, (n, k), np.float32, x)
        I = self._out(I, (n, k), np.int64, x)
        pD, _c = _out_ptr(D, np.float32)
        pI, _d = _out_ptr(I, np.int64)
        check(lib().vlq_ivfpq_refine(self._h, C.c_int64(n), px, ps, C.c_int(k_coarse), C.c_int(k), pD, pI))
        return D, I

    def search_refined(self, x, nprobe, k, k_factor, D=None, I=None):
        """IndexIVFPQR::search: first stage at k_coarse = long(k * k_factor), then the refine stage"""
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        D = self._out(D, (n, k), np.float32, x)
        I = self._out(I, (n, k), np.int64, x)
        pD, _b = _out_ptr(D, np.float32)
        pI, _c = _out_ptr(I, np.int64)
        check(lib().vlq_ivfpq_search_refined(self._h, C.c_int64(n), px, C.c_int(nprobe), C.c_int(k), C.c_float(k_factor), pD, pI))
        return D, I

    def search_refined_preassigned(self, x, keys, coarse_dis, k, k_factor, D=None, I=None):
        n = x.shape[0]
        nprobe = keys.shape[1]
        px, _a = _ptr(x, np.float32)
        pk, _b = _ptr(keys, np.int64)
        pc, _c = _ptr(coarse_dis, np.float32)
        D = self._out(D, (n, k), np.float32, x)
        I = self._out(I, (n, k), np.int64, x)
        pD, _d = _out_ptr(D, np.float32)
        pI, _e = _out_ptr(I, np.int64)
        check(lib().vlq_ivfpq_search_refined_preassigned(self._h, C.c_int64(n), px, pk, pc, C.c_int(nprobe), C.c_int(k),
                                                         C.c_float(k_factor), pD, pI))
        return D, I

    # --- introspection ----------------------------------------------------
    def query_tables(self, x, inner_product=True):
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        out = np.empty((n, self.M, self.ksub), np.float32)
        check(lib().vlq_ivfpq_query_tables(self._h, C.c_int64(n), px, C.c_int(int(inner_product)),
                                           out.ctypes.data_as(C.c_void_p)))
        return out

    def query_codes(self, x, keys):
        """q_code [n][nprobe][M] the polysemous filter compares the stored codes of every (query, probe) with"""
        n, nprobe = x.shape[0], keys.shape[1]
        px, _a = _ptr(x, np.float32)
        pk, _b = _ptr(keys, np.int64)
        out = np.empty((n, nprobe, self.M), np.uint8)
        check(lib().vlq_ivfpq_query_codes(self._h, C.c_int64(n), px, pk, C.c_int(nprobe), out.ctypes.data_as(C.c_void_p)))
        return out

    def polysemous_stats(self, reset=False):
        """indexIVFPQ_stats.n_hamming_pass: codes that passed the Hamming filter since the last reset"""
        n = C.c_uint64()
        check(lib().vlq_ivfpq_polysemous_stats(self._h, C.byref(n), C.c_int(int(reset))))
        return n.value

    def precomputed_table(self, rows=None):
        out = np.empty((rows or self.nlist, self.M, self.ksub), np.float32)
        check(lib().vlq_ivfpq_get_precomputed_table(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def stats(self, reset=False):
        nq, ncode = C.c_uint64(), C.c_uint64()
        check(lib().vlq_ivfpq_stats(self._h, C.byref(nq), C.byref(ncode), C.c_int(int(reset))))
        return nq.value, ncode.value

    def last_scan_info(self):
        """what the last search's list scan was (kernel shape, walking order, clock period): include/vlq_ivfpq.h"""
        buf = C.create_string_buffer(256)
        check(lib().vlq_ivfpq_last_scan_info(self._h, buf, C.c_int(256)))
        return buf.value.decode()

    def reset_walk_state(self):
        check(lib().vlq_ivfpq_reset_walk_state(self._h))

    def profile(self, enable=True):
        """0 / False: off; 1 / True: every stage; 2: the scan kernel only (two event records per call);
        3: the scan kernel of every 4th call, starting with the next one"""
        check(lib().vlq_ivfpq_profile(self._h, C.c_int(int(enable))))

    def profile_read(self, reset=True):
        ms = (C.c_double * 3)()
        calls = C.c_int64()
        check(lib().vlq_ivfpq_profile_read(self._h, ms, C.byref(calls), C.c_int(int(reset))))
        return {"coarse_ms": ms[0], "tables_ms": ms[1], "scan_ms": ms[2], "scan_calls": calls.value}


class _GpuIVF:
    """What GpuIVFFlat and GpuIVFSQ share: the calls of the C ABI that differ in their prefix only (_KIND)."""

    METRICS = GpuIVFPQ.METRICS
    _KIND = None
    _out = GpuIVFPQ._out

    def _call(self, name, *args):
        check(getattr(lib(), self._KIND + name)(self._h, *args))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(lib(), self._KIND + "destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- state ------------------------------------------------------------
    def set_stream(self, stream_ptr):
        self._call("set_stream", C.c_void_p(stream_ptr or 0))

    def set_coarse_centroids(self, c):
        p, _k = _ptr(c, np.float32)
        self._call("set_coarse_centroids", p)

    def _set_lists(self, rows, np_dtype, ids, list_offsets):
        pv, _a = _ptr(rows, np_dtype)
        pi, _b = _ptr(ids, np.int64)
        po, _c = _ptr(list_offsets, np.int64)
        self._call("set_lists", pv, pi, po)

    @property
    def ntotal(self):
        return int(getattr(lib(), self._KIND + "ntotal")(self._h))

    def list_length(self, i):
        n = C.c_int64()
        self._call("list_length", C.c_int(i), C.byref(n))
        return n.value

    def _get_list(self, i, width, np_dtype):
        rows = np.empty((self.list_length(i), width), np_dtype)
        ids = np.empty((rows.shape[0],), np.int64)
        self._call("get_list", C.c_int(i), rows.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p))
        return rows, ids

    def reset(self):
        self._call("reset")

    # --- add --------------------------------------------------------------
    def add(self, x, xids=None):
        px, _a = _ptr(x, np.float32)
        pi, _b = _ptr(xids, np.int64)
        self._call("add", C.c_int64(x.shape[0]), px, pi)

    def add_preassigned(self, x, assign, xids=None):
        px, _a = _ptr(x, np.float32)
        pi, _b = _ptr(xids, np.int64)
        pa, _c = _ptr(assign, np.int64)
        self._call("add_preassigned", C.c_int64(x.shape[0]), px, pi, pa)

    def reserve_memory(self, num_vecs):
        self._call("reserve_memory", C.c_int64(num_vecs))

    def reclaim_memory(self):
        n = C.c_uint64()
        self._call("reclaim_memory", C.byref(n))
        return n.value

    # --- search -----------------------------------------------------------
    def _rows_out(self, x, width, D, I):
        """the two outputs of a search of x, [n][width] float32 and int64, with their pointers"""
        D = self._out(D, (x.shape[0], width), np.float32, x)
        I = self._out(I, (x.shape[0], width), np.int64, x)
        return D, I, _out_ptr(D, np.float32)[0], _out_ptr(I, np.int64)[0]

    def search(self, x, nprobe, k, D=None, I=None):
        px, _a = _ptr(x, np.float32)
        D, I, pD, pI = self._rows_out(x, k, D, I)
        self._call("search", C.c_int64(x.shape[0]), px, C.c_int(nprobe), C.c_int(k), pD, pI)
        return D, I

    def coarse_search(self, x, nprobe, cdis=None, keys=None):
        px, _a = _ptr(x, np.float32)
        cdis, keys, pc, pk = self._rows_out(x, nprobe, cdis, keys)
        self._call("coarse_search", C.c_int64(x.shape[0]), px, C.c_int(nprobe), pc, pk)
        return cdis, keys

    # --- introspection ----------------------------------------------------
    def last_scan_info(self):
        buf = C.create_string_buffer(256)
        self._call("last_scan_info", buf, C.c_int(256))
        return buf.value.decode()


class GpuIVFFlat(_GpuIVF):
    """faiss::IndexIVFFlat / gpu::GpuIndexIVFFlat (IndexIVF.h:132-205, gpu/GpuIndexIVFFlat.h): inverted lists of the vectors
    themselves, exact distances.  metric "l2": ascending squared distances, FLT_MAX / -1 padding; "ip": descending inner
    products, -FLT_MAX / -1 padding (include/vlq_ivfpq.h, vlq_ivfflat_*)."""

    _KIND = "vlq_ivfflat_"

    def __init__(self, d, nlist, device=0, metric="l2"):
        self.d, self.nlist, self.device = d, nlist, device
        self._h = C.c_void_p()
        if metric not in self.METRICS:
            raise ValueError("metric %r (one of 'l2', 'ip')" % (metric,))
        self.metric = metric
        check(lib().vlq_ivfflat_create(C.byref(self._h), C.c_int(device), C.c_int(d), C.c_int(nlist), C.c_int(self.METRICS[metric])))

    def set_lists(self, vecs, ids, list_offsets):
        """vecs [ntotal][d] float32 and ids [ntotal] in list-contiguous order, list_offsets [nlist + 1]"""
        self._set_lists(vecs, np.float32, ids, list_offsets)

    def get_list(self, i):
        return self._get_list(i, self.d, np.float32)

    def add_preassigned(self, x, assign, xids=None):
        """IndexIVFFlat::add_core with precomputed_idx: a negative list id drops the vector"""
        super().add_preassigned(x, assign, xids)

    def search_preassigned(self, x, keys, k, D=None, I=None):
        px, _a = _ptr(x, np.float32)
        pk, _b = _ptr(keys, np.int64)
        D, I, pD, pI = self._rows_out(x, k, D, I)
        self._call("search_preassigned", C.c_int64(x.shape[0]), px, pk, C.c_int(keys.shape[1]), C.c_int(k), pD, pI)
        return D, I

    def reset(self):
        super().reset()
        self._range_total = 0

    # --- range search -----------------------------------------------------
    def _range(self, name, x, *args):
        """(lims [n + 1], D [total], I [total]) of a range search of x: outputs on x's device if x is a device tensor.  The radius
        goes as a C float: the loader sets no argtypes, and a bare Python float would be passed as a double."""
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        lims = self._out(None, (n + 1,), np.int64, x)
        total = C.c_int64()
        self._range_total = 0          # (a failed call leaves an empty result in the handle)
        self._call(name, C.c_int64(n), px, *args, _out_ptr(lims, np.int64)[0], C.byref(total))
        self._range_total = total.value
        return (lims,) + self.range_result(like=x)

    def range_search(self, x, nprobe, radius):
        """IndexIVFFlat::range_search: every stored vector of the nprobe nearest lists with dis < radius ("l2") or ip > radius
        ("ip"), per query in scan order (probe order, then list position); query i's hits are D / I [lims[i]:lims[i + 1]]"""
        return self._range("range_search", x, C.c_int(nprobe), C.c_float(radius))

    def range_search_preassigned(self, x, keys, radius):
        """the same from the caller's probes keys [n][nprobe]; a key < 0 or >= nlist is an error (the reference aborts)"""
        pk, _b = _ptr(keys, np.int64)
        return self._range("range_search_preassigned", x, pk, C.c_int(keys.shape[1]), C.c_float(radius))

    def range_result(self, like=None):
        """(D, I) of the last range search again (held until the next range search, reset or close); device tensors if
        `like` is one"""
        total = getattr(self, "_range_total", 0)
        D = self._out(None, (total,), np.float32, like)
        I = self._out(None, (total,), np.int64, like)
        self._call("range_result", _out_ptr(D, np.float32)[0], _out_ptr(I, np.int64)[0])
        return D, I

    def stats(self, reset=False):
        """IndexIVFFlatStats since the last reset: (nq, lists visited, distances computed)"""
        nq, nl, nd = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._call("stats", C.byref(nq), C.byref(nl), C.byref(nd), C.c_int(int(reset)))
        return nq.value, nl.value, nd.value

    def last_scan_info(self):
        """the kernel instantiation and read path of the last list scan (include/vlq_ivfpq.h)"""
        return super().last_scan_info()


class GpuIVFSQ(_GpuIVF):
    """faiss::IndexIVFScalarQuantizer (IndexScalarQuantizer.h:129-155; "IVFx,SQ8" / "IVFx,SQ4" of index_factory): inverted
    lists of 8- or 4-bit codes per component of the residual.  qtype: "8bit", "4bit", "8bit_uniform", "4bit_uniform" (or
    ScalarQuantizer::QuantizerType's number).  metric "l2": ascending distances, FLT_MAX / -1 padding; "ip": descending inner
    products, -FLT_MAX / -1 padding (include/vlq_ivfpq.h, vlq_ivfsq_*)."""

    _KIND = "vlq_ivfsq_"
    QTYPES = {"8bit": 0, "4bit": 1, "8bit_uniform": 2, "4bit_uniform": 3}      # ScalarQuantizer::QuantizerType

    def __init__(self, d, nlist, qtype, device=0, metric="l2"):
        self.d, self.nlist, self.device = d, nlist, device
        self._h = C.c_void_p()
        if metric not in self.METRICS:
            raise ValueError("metric %r (one of 'l2', 'ip')" % (metric,))
        qt = self.QTYPES.get(qtype, qtype)
        if qt not in self.QTYPES.values():
            raise ValueError("qtype %r (one of %s)" % (qtype, ", ".join(repr(s) for s in self.QTYPES)))
        self.metric, self.qtype = metric, int(qt)
        self.uniform = self.qtype >= 2
        self.bits = 8 if self.qtype in (0, 2) else 4
        check(lib().vlq_ivfsq_create(C.byref(self._h), C.c_int(device), C.c_int(d), C.c_int(nlist), C.c_int(self.qtype),
                                     C.c_int(self.METRICS[metric])))
        self.code_size = int(lib().vlq_ivfsq_code_size(self._h))

    def set_coarse_centroids(self, c):
        super().set_coarse_centroids(c)
        # train() takes the residuals on the host
        host = c.detach().cpu().numpy() if _is_torch(c) else c
        self._centroids = np.array(host, dtype=np.float32).reshape(self.nlist, self.d)

    def set_trained(self, trained):
        """ScalarQuantizer::trained: vmin[d] then vdiff[d] (two floats for the uniform types), host floats"""
        t = np.ascontiguousarray(np.asarray(trained, dtype=np.float32).ravel())
        self._call("set_trained", t.ctypes.data_as(C.c_void_p), C.c_int(t.size))

    @property
    def trained(self):
        t = np.empty(2 if self.uniform else 2 * self.d, np.float32)
        self._call("get_trained", t.ctypes.data_as(C.c_void_p), C.c_int(t.size))
        return t

    def train(self, x):
        """IndexIVFScalarQuantizer::train_residual with the constructor's RS_minmax, rangestat_arg 0
        (IndexScalarQuantizer.cpp:824-839, :270-286, :369-392): the 1-NN assignment runs on the device, the residuals and their
        minima / maxima are taken in float32 on the host."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        _cd, keys = self.coarse_search(x, 1)
        if (keys < 0).any():
            raise ValueError("a training vector has no nearest centroid")
        cent = self._centroids
        res = x - cent[keys[:, 0]]
        if self.uniform:
            vmin, vmax = res.min(), res.max()
        else:
            vmin, vmax = res.min(axis=0), res.max(axis=0)
        self.set_trained(np.concatenate([np.atleast_1d(vmin), np.atleast_1d((vmax - vmin).astype(np.float32))]))

    def set_lists(self, codes, ids, list_offsets):
        """codes [ntotal][code_size] uint8 and ids [ntotal] in list-contiguous order, list_offsets [nlist + 1]"""
        self._set_lists(codes, np.uint8, ids, list_offsets)

    def get_list(self, i):
        return self._get_list(i, self.code_size, np.uint8)

    def add_preassigned(self, x, assign, xids=None):
        """add_with_ids behind a given assignment: a negative list id drops the vector"""
        super().add_preassigned(x, assign, xids)

    def encode(self, x):
        """(codes [n][code_size], assignment [n]) that add would store; nothing is stored"""
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        codes = np.empty((n, self.code_size), np.uint8)
        assign = np.empty((n,), np.int64)
        self._call("encode", C.c_int64(n), px, codes.ctypes.data_as(C.c_void_p), assign.ctypes.data_as(C.c_void_p))
        return codes, assign

    def search_preassigned(self, x, keys, coarse_dis, k, D=None, I=None):
        """coarse_dis [n][nprobe] is read under inner product only and may be None for L2"""
        px, _a = _ptr(x, np.float32)
        pk, _b = _ptr(keys, np.int64)
        pc, _f = _ptr(coarse_dis, np.float32)
        D, I, pD, pI = self._rows_out(x, k, D, I)
        self._call("search_preassigned", C.c_int64(x.shape[0]), px, pk, pc, C.c_int(keys.shape[1]), C.c_int(k), pD, pI)
        return D, I

    def last_scan_info(self):
        """the kernel instantiation and read path of the last list scan (include/vlq_ivfpq.h); raises a pending bad-key error"""
        return super().last_scan_info()


class _GpuOneList:
    """What GpuPQ, GpuSQ, GpuFlat and GpuLSH share: the calls of the C ABI that differ in their prefix only (_PREFIX) -- the
    handle's lifetime and stream, add, ntotal, reset, reserve_memory, search(x, k) and last_scan_info (csrc/one_list.h)."""

    _PREFIX = None
    _out = GpuIVFPQ._out

    def _call(self, name, *args):
        check(getattr(lib(), self._PREFIX + name)(self._h, *args))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(lib(), self._PREFIX + "destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        self._call("set_stream", C.c_void_p(stream_ptr or 0))

    def add(self, x):
        px, _a = _ptr(x, np.float32)
        self._call("add", C.c_int64(x.shape[0]), px)

    @property
    def ntotal(self):
        return int(getattr(lib(), self._PREFIX + "ntotal")(self._h))

    def reset(self):
        self._call("reset")

    def reserve_memory(self, num_vecs):
        self._call("reserve_memory", C.c_int64(num_vecs))

    def search(self, x, k, D=None, I=None):
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        D = self._out(D, (n, k), np.float32, x)
        I = self._out(I, (n, k), np.int64, x)
        self._call("search", C.c_int64(n), px, C.c_int(k), _out_ptr(D, np.float32)[0], _out_ptr(I, np.int64)[0])
        return D, I

    def last_scan_info(self):
        buf = C.create_string_buffer(256)
        self._call("last_scan_info", buf, C.c_int(256))
        return buf.value.decode()


class GpuPQ(_GpuOneList):
    """faiss::IndexPQ (IndexPQ.h:28-117; "PQx" of index_factory): every stored code is scored for every query.  metric "l2":
    ascending distances, FLT_MAX / -1 padding; "ip": descending inner products, -FLT_MAX / -1 padding.  Labels are scan
    positions.  search_type: "pq" (ADC), "sdc", "polysemous", "polysemous_generalize", or Search_type_t's number
    (include/vlq_ivfpq.h, vlq_pq_*)."""

    METRICS = GpuIVFPQ.METRICS
    SEARCH_TYPES = {"pq": 0, "he": 1, "generalized_he": 2, "sdc": 3, "polysemous": 4, "polysemous_generalize": 5}   # IndexPQ::Search_type_t
    _PREFIX = "vlq_pq_"

    def __init__(self, d, M, nbits=8, metric="l2", device=0):
        self.d, self.M, self.nbits, self.device = d, M, nbits, device
        self.ksub = 1 << nbits
        self._h = C.c_void_p()
        if metric not in self.METRICS:
            raise ValueError("metric %r (one of 'l2', 'ip')" % (metric,))
        self.metric = metric
        check(lib().vlq_pq_create(C.byref(self._h), C.c_int(device), C.c_int(d), C.c_int(M), C.c_int(nbits), C.c_int(self.METRICS[metric])))
        self._search_type = 0
        self._polysemous_ht = nbits * M + 1

    # --- state ------------------------------------------------------------
    def set_centroids(self, c):
        """ProductQuantizer::centroids [M][ksub][dsub]"""
        p, _k = _ptr(c, np.float32)
        self._call("set_centroids", p)

    def set_codes(self, codes):
        """IndexPQ::codes [ntotal][M] uint8; replaces the stored codes"""
        p, _k = _ptr(codes, np.uint8)
        self._call("set_codes", p, C.c_int64(codes.shape[0]))

    def encode(self, x):
        """the codes [n][M] add would store; nothing is stored"""
        px, _a = _ptr(x, np.float32)
        codes = np.empty((x.shape[0], self.M), np.uint8)
        self._call("encode", C.c_int64(x.shape[0]), px, codes.ctypes.data_as(C.c_void_p))
        return codes

    def codes(self, i0=0, ni=None):
        """stored codes i0 .. i0 + ni - 1 in scan order, [ni][M] uint8"""
        ni = self.ntotal - i0 if ni is None else ni
        out = np.empty((ni, self.M), np.uint8)
        self._call("get_codes", C.c_int64(i0), C.c_int64(ni), out.ctypes.data_as(C.c_void_p))
        return out

    def _set_search(self, search_type, ht):
        st = self.SEARCH_TYPES.get(search_type, search_type)
        if st not in self.SEARCH_TYPES.values():
            raise ValueError("search type %r (one of %s)" % (search_type, ", ".join(repr(s) for s in self.SEARCH_TYPES)))
        self._call("set_search_type", C.c_int(int(st)), C.c_int(int(ht)))
        self._search_type, self._polysemous_ht = int(st), int(ht)

    @property
    def search_type(self):
        return self._search_type

    @search_type.setter
    def search_type(self, search_type):
        self._set_search(search_type, self._polysemous_ht)

    @property
    def polysemous_ht(self):
        return self._polysemous_ht

    @polysemous_ht.setter
    def polysemous_ht(self, ht):
        self._set_search(self._search_type, ht)

    # --- search -----------------------------------------------------------
    def query_tables(self, x):
        """the tables the scan reads for x, [n][M][ksub] float32"""
        px, _a = _ptr(x, np.float32)
        out = np.empty((x.shape[0], self.M, self.ksub), np.float32)
        self._call("query_tables", C.c_int64(x.shape[0]), px, out.ctypes.data_as(C.c_void_p))
        return out

    def query_codes(self, x):
        """the queries' codes the polysemous filter / SDC reads, [n][M] uint8"""
        px, _a = _ptr(x, np.float32)
        out = np.empty((x.shape[0], self.M), np.uint8)
        self._call("query_codes", C.c_int64(x.shape[0]), px, out.ctypes.data_as(C.c_void_p))
        return out

    def stats(self, reset=False):
        """IndexPQStats since the last reset: (nq, ncode, n_hamming_pass)"""
        nq, nc, nh = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._call("stats", C.byref(nq), C.byref(nc), C.byref(nh), C.c_int(int(reset)))
        return nq.value, nc.value, nh.value

    def set_scan_split(self, query_tile=0, slices=0):
        """speed only: queries per workgroup (0, 1, 2, 4) and code slices (0 .. 64); 0 = the plan decides"""
        self._call("set_scan_split", C.c_int(query_tile), C.c_int(slices))


class GpuSQ(_GpuOneList):
    """faiss::IndexScalarQuantizer (IndexScalarQuantizer.h:82-120; "SQ8" / "SQ4" of index_factory): every stored code of 8 or 4
    bits per component is decoded and compared with every query.  qtype as for GpuIVFSQ.  The reference leaves its rows in
    heap order (it never reorders the heap in this search); here they come back sorted: metric "l2": ascending distances, then
    ascending positions, FLT_MAX / -1 padding; "ip": descending inner products, -FLT_MAX / -1 padding.  Labels are scan
    positions (include/vlq_ivfpq.h, vlq_sq_*)."""

    METRICS = GpuIVFPQ.METRICS
    QTYPES = GpuIVFSQ.QTYPES
    _PREFIX = "vlq_sq_"

    def __init__(self, d, qtype, device=0, metric="l2"):
        self.d, self.device = d, device
        self._h = C.c_void_p()
        if metric not in self.METRICS:
            raise ValueError("metric %r (one of 'l2', 'ip')" % (metric,))
        qt = self.QTYPES.get(qtype, qtype)
        self.metric, self.qtype = metric, int(qt)
        check(lib().vlq_sq_create(C.byref(self._h), C.c_int(device), C.c_int(d), C.c_int(self.qtype), C.c_int(self.METRICS[metric])))
        self.uniform = self.qtype >= 2
        self.bits = 8 if self.qtype in (0, 2) else 4
        self.code_size = int(lib().vlq_sq_code_size(self._h))

    def set_trained(self, trained):
        """ScalarQuantizer::trained: vmin[d] then vdiff[d] (two floats for the uniform types), host floats"""
        t = np.ascontiguousarray(np.asarray(trained, dtype=np.float32).ravel())
        self._call("set_trained", t.ctypes.data_as(C.c_void_p), C.c_int(t.size))

    @property
    def trained(self):
        t = np.empty(2 if self.uniform else 2 * self.d, np.float32)
        self._call("get_trained", t.ctypes.data_as(C.c_void_p), C.c_int(t.size))
        return t

    def train(self, x):
        """IndexScalarQuantizer::train (IndexScalarQuantizer.cpp:713-717) with the constructor's RS_minmax, rangestat_arg 0
        (:270-286, :369-392): the minima / maxima of x itself, taken in float32 on the host."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if self.uniform:
            vmin, vmax = x.min(), x.max()
        else:
            vmin, vmax = x.min(axis=0), x.max(axis=0)
        self.set_trained(np.concatenate([np.atleast_1d(vmin), np.atleast_1d((vmax - vmin).astype(np.float32))]))

    def set_codes(self, codes):
        """IndexScalarQuantizer::codes [ntotal][code_size] uint8; replaces the stored codes"""
        p, _k = _ptr(codes, np.uint8)
        self._call("set_codes", p, C.c_int64(codes.shape[0]))

    def encode(self, x):
        """the codes [n][code_size] add would store; nothing is stored"""
        px, _a = _ptr(x, np.float32)
        codes = np.empty((x.shape[0], self.code_size), np.uint8)
        self._call("encode", C.c_int64(x.shape[0]), px, codes.ctypes.data_as(C.c_void_p))
        return codes

    def codes(self, i0=0, n=None):
        """stored codes i0 .. i0 + n - 1 in scan order, [n][code_size] uint8"""
        n = self.ntotal - i0 if n is None else n
        out = np.empty((n, self.code_size), np.uint8)
        self._call("get_codes", C.c_int64(i0), C.c_int64(n), out.ctypes.data_as(C.c_void_p))
        return out

    def reconstruct_n(self, i0=0, n=None, out=None):
        """IndexScalarQuantizer::reconstruct_n: the decoded vectors i0 .. i0 + n - 1, [n][d] float32 (out: a numpy array or a
        torch tensor to fill)"""
        n = self.ntotal - i0 if n is None else n
        if out is None:
            out = np.empty((n, self.d), np.float32)
        self._call("reconstruct", C.c_int64(i0), C.c_int64(n), _out_ptr(out, np.float32)[0])
        return out

    def set_scan_split(self, query_tile=0, slices=0):
        """speed only: queries per workgroup (0, 1, 2, 4) and code slices (0 .. 64); 0 = the plan decides"""
        self._call("set_scan_split", C.c_int(query_tile), C.c_int(slices))


class GpuFlat(_GpuOneList):
    """faiss::IndexFlat / IndexFlatL2 / IndexFlatIP (gpu::GpuIndexFlat): the exact brute-force index.  metric "l2": ascending
    squared distances, FLT_MAX / -1 padding; "ip": descending inner products, -FLT_MAX / -1 padding.  Labels are positions in
    the order of add.  Fewer than 20 queries with d % 4 == 0 take the reference's per-pair SSE order, everything else the fmaf
    chain of the GEMM path; the call's n decides, never a page's (include/vlq_ivfpq.h, vlq_flat_*)."""

    METRICS = GpuIVFPQ.METRICS
    _PREFIX = "vlq_flat_"

    def __init__(self, d, metric="l2", device=0):
        self.d, self.device = d, device
        self._h = C.c_void_p()
        if metric not in self.METRICS:
            raise ValueError("metric %r (one of 'l2', 'ip')" % (metric,))
        self.metric = metric
        check(lib().vlq_flat_create(C.byref(self._h), C.c_int(device), C.c_int(d), C.c_int(self.METRICS[metric])))
        self._range_total = 0         # hits the handle holds (range_search)

    def reconstruct_n(self, i0=0, n=None, out=None):
        """the stored bits of vectors i0 .. i0 + n - 1, [n][d] float32 (out: a numpy array or a torch tensor to fill)"""
        n = self.ntotal - i0 if n is None else n
        if out is None:
            out = np.empty((n, self.d), np.float32)
        self._call("reconstruct_n", C.c_int64(i0), C.c_int64(n), _out_ptr(out, np.float32)[0])
        return out

    def scan_split(self, row_tile=0, slices=0):
        """speed only: query rows per workgroup of the fused scan (0, 32, 64, 128) and column slices (0 .. 64); 0 = the plan decides"""
        self._call("set_scan_split", C.c_int(row_tile), C.c_int(slices))

    def reset(self):
        super().reset()
        self._range_total = 0

    # --- range search (IndexFlat.cpp:58-70) -------------------------------------
    def range_search(self, x, radius):
        """IndexFlat::range_search: every stored vector with dis < radius ("l2") or ip > radius ("ip"), per query in ascending
        position; (lims [n + 1], D [total], I [total]), query i's hits are D / I [lims[i]:lims[i + 1]].  Outputs are on x's
        device if x is a device tensor.  The radius goes as a C float: the loader sets no argtypes, and a bare Python float
        would be passed as a double."""
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        lims = self._out(None, (n + 1,), np.int64, x)
        total = C.c_int64()
        self._range_total = 0          # (a failed call leaves an empty result in the handle)
        self._call("range_search", C.c_int64(n), px, C.c_float(radius), _out_ptr(lims, np.int64)[0], C.byref(total))
        self._range_total = total.value
        return (lims,) + self.range_result(like=x)

    def range_result(self, like=None):
        """(D, I) of the last range search again (held until the next range search, reset or close); device tensors if
        `like` is one"""
        total = self._range_total
        D = self._out(None, (total,), np.float32, like)
        I = self._out(None, (total,), np.int64, like)
        self._call("range_result", _out_ptr(D, np.float32)[0], _out_ptr(I, np.int64)[0])
        return D, I

    # --- IndexRefineFlat's seam (IndexFlat.cpp:73-93, :245-260) -----------------
    def compute_distance_subset(self, x, labels, distances):
        """IndexFlat::compute_distance_subset: distances [n][k] (written in place, returned) becomes the distance of x[i] to
        the vector at position labels[i][j]; entries whose label is < 0 are left untouched"""
        n, k = labels.shape
        px, _a = _ptr(x, np.float32)
        pl, _b = _ptr(labels, np.int64)
        self._call("compute_distance_subset", C.c_int64(n), px, C.c_int(k), _out_ptr(distances, np.float32)[0], pl)
        return distances

    def refine(self, x, base_D, base_I, k, D=None, I=None):
        """lines 245-260 of IndexRefineFlat::search: the shortlist base_D / base_I [n][k_base] (labels = positions, < 0 = skip)
        re-scored exactly and the best k kept.  D / I may be base_D / base_I when k == k_base."""
        n, k_base = base_I.shape
        px, _a = _ptr(x, np.float32)
        pd, _b = _ptr(base_D, np.float32)
        pl, _c = _ptr(base_I, np.int64)
        D = self._out(D, (n, k), np.float32, x)
        I = self._out(I, (n, k), np.int64, x)
        self._call("refine", C.c_int64(n), px, C.c_int(k_base), pd, pl, C.c_int(k), _out_ptr(D, np.float32)[0], _out_ptr(I, np.int64)[0])
        return D, I

    def last_refine_info(self):
        buf = C.create_string_buffer(256)
        self._call("last_refine_info", buf, C.c_int(256))
        return buf.value.decode()


def random_rotation(d, nbits, seed=5):
    """A random rotation [nbits][d] float32 in LinearTransform's layout (xt = A x): numpy's generator seeded with `seed`, then
    a QR.  nbits <= d: the first nbits rows of an orthonormal d x d matrix; nbits > d: the first d columns of an orthonormal
    nbits x nbits one.  This is A random rotation, NOT the bits of the reference's RandomRotationMatrix::init(seed): those come
    from its own float_randn and LAPACK's sgeqrf / sorgqr.  An index that must reproduce the reference's codes takes the
    reference's matrix as data (GpuLSH.set_rotation)."""
    m = max(d, nbits)
    q, _r = np.linalg.qr(np.random.default_rng(seed).standard_normal((m, m)))
    return np.ascontiguousarray(q[:nbits, :d], dtype=np.float32)


class GpuLSH(_GpuOneList):
    """faiss::IndexLSH (IndexLSH.h; "LSH" of index_factory): a vector becomes the sign bits of its (optionally rotated,
    optionally thresholded) components, search is the exhaustive Hamming scan.  Distances are the integer Hamming distances as
    float32, ascending by (distance, position), padded 2147483648.0 / -1.  Labels are positions in the order of add.
    With rotate_data and no set_rotation call the matrix is random_rotation(d, nbits, seed=5): a random rotation, NOT the
    reference's bits (include/vlq_ivfpq.h, vlq_lsh_*)."""

    metric = "l2"         # what a GpuRefineFlat over this index re-ranks by
    _PREFIX = "vlq_lsh_"

    def __init__(self, d, nbits, rotate_data=True, train_thresholds=False, device=0):
        self.d, self.nbits, self.device = d, nbits, device
        self.rotate_data, self.train_thresholds = bool(rotate_data), bool(train_thresholds)
        self.bytes_per_vec = (nbits + 7) // 8
        self._h = C.c_void_p()
        check(lib().vlq_lsh_create(C.byref(self._h), C.c_int(device), C.c_int(d), C.c_int(nbits), C.c_int(int(self.rotate_data)),
                                   C.c_int(int(self.train_thresholds))))
        self.is_trained = not self.train_thresholds
        if self.rotate_data:
            self.set_rotation(random_rotation(d, nbits, seed=5))

    # --- state ------------------------------------------------------------
    def set_rotation(self, A, b=None):
        """rrot.A [nbits][d] and rrot.b [nbits] (None: no bias)"""
        pa, _a = _ptr(A, np.float32)
        pb, _b = _ptr(b, np.float32)
        self._call("set_rotation", pa, pb)

    def set_thresholds(self, t):
        """IndexLSH::thresholds [nbits]; None: back to untrained"""
        pt, _t = _ptr(t, np.float32)
        self._call("set_thresholds", pt)
        self.is_trained = t is not None or not self.train_thresholds

    def train(self, x):
        """IndexLSH::train (IndexLSH.cpp:85-113): the rotation runs on the device, the per-bit median is taken here -- the sorted
        column's element n/2 for odd n, (x[n/2-1] + x[n/2]) / 2 in float32 for even n.  Returns the thresholds."""
        if not self.train_thresholds:
            self.is_trained = True
            return None
        self.set_thresholds(None)
        xt = self.apply(x)
        xt = np.sort(xt.cpu().numpy() if _is_torch(xt) else xt, axis=0)
        n = xt.shape[0]
        if n % 2 == 1:
            t = xt[n // 2].copy()
        else:
            t = ((xt[n // 2 - 1] + xt[n // 2]) / np.float32(2)).astype(np.float32)
        self.set_thresholds(t)
        return t

    def apply(self, x, out=None):
        """apply_preprocess: [n][nbits] float32 (thresholds are subtracted once they are set)"""
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        out = self._out(out, (n, self.nbits), np.float32, x)
        self._call("apply", C.c_int64(n), px, _out_ptr(out, np.float32)[0])
        return out

    def encode(self, x):
        """the codes [n][bytes_per_vec] add would store; nothing is stored"""
        px, _a = _ptr(x, np.float32)
        codes = np.empty((x.shape[0], self.bytes_per_vec), np.uint8)
        self._call("encode", C.c_int64(x.shape[0]), px, codes.ctypes.data_as(C.c_void_p))
        return codes

    def add_codes(self, codes):
        """ready-made codes [n][bytes_per_vec] uint8, appended as they are"""
        if codes.shape[1] != self.bytes_per_vec:
            raise ValueError("codes of %d bytes for an index of %d" % (codes.shape[1], self.bytes_per_vec))
        pc, _c = _ptr(codes, np.uint8)
        self._call("add_codes", C.c_int64(codes.shape[0]), pc)

    def get_codes(self, i0=0, ni=None):
        """stored codes i0 .. i0 + ni - 1, [ni][bytes_per_vec] uint8"""
        ni = self.ntotal - i0 if ni is None else ni
        out = np.empty((ni, self.bytes_per_vec), np.uint8)
        self._call("get_codes", C.c_int64(i0), C.c_int64(ni), out.ctypes.data_as(C.c_void_p))
        return out

    # --- search -----------------------------------------------------------
    def search_codes(self, qcodes, k, D=None, I=None):
        """hammings_knn of ready-made query codes [n][bytes_per_vec] uint8"""
        n = qcodes.shape[0]
        if qcodes.shape[1] != self.bytes_per_vec:
            raise ValueError("codes of %d bytes for an index of %d" % (qcodes.shape[1], self.bytes_per_vec))
        pq, _a = _ptr(qcodes, np.uint8)
        D = self._out(D, (n, k), np.float32, qcodes)
        I = self._out(I, (n, k), np.int64, qcodes)
        self._call("search_codes", C.c_int64(n), pq, C.c_int(k), _out_ptr(D, np.float32)[0], _out_ptr(I, np.int64)[0])
        return D, I

    def scan_split(self, query_tile=0, slices=0):
        """speed only: queries per workgroup (0, 1, 2, 4) and code slices (0 .. 64); 0 = the plan decides"""
        self._call("set_scan_split", C.c_int(query_tile), C.c_int(slices))


VLQ_MAX_K = 1024      # include/vlq_ivfpq.h


class GpuRefineFlat:
    """faiss::IndexRefineFlat (IndexFlat.h:103-140): a base index whose shortlist of k * k_factor candidates is re-scored
    exactly against the uncompressed vectors kept beside it.  base: GpuIVFPQ, GpuIVFFlat, GpuIVFSQ, GpuPQ, GpuSQ, GpuFlat or GpuLSH; the
    refine store is a GpuFlat of the base's d and metric.  A base label must be a position in the store: add() keeps the two in
    step (IVF bases get the sequential ids ntotal .. ntotal + n - 1); an index whose lists were set with ids 0 .. ntotal - 1
    gets its store from set_store().  The base and the store share one stream of this object's (set_stream replaces it), so the
    shortlist of a device-side query never leaves the device."""

    def __init__(self, base):
        import torch
        if not isinstance(base, (GpuIVFPQ, GpuIVFFlat, GpuIVFSQ, GpuPQ, GpuSQ, GpuFlat, GpuLSH)):
            raise TypeError("base must be a GpuIVFPQ, GpuIVFFlat, GpuIVFSQ, GpuPQ, GpuSQ, GpuFlat or GpuLSH, got %s" % type(base).__name__)
        self.base = base
        self.d, self.metric, self.device = base.d, base.metric, base.device
        self.k_factor = 1.0
        self.nprobe = 1           # IndexIVF's default, used where search() is given none
        self.store = GpuFlat(self.d, metric=self.metric, device=self.device)
        self._ivf = isinstance(base, (GpuIVFPQ, _GpuIVF))
        self._dev = torch.device("cuda", self.device)
        self._stream = torch.cuda.Stream(device=self._dev)
        self.set_stream(self._stream.cuda_stream)
        self._short = None        # (D, I) device tensors of the last shortlist, reused while the shape holds

    def set_stream(self, stream_ptr):
        self.base.set_stream(stream_ptr)
        self.store.set_stream(stream_ptr)

    @property
    def ntotal(self):
        return self.store.ntotal

    def add(self, x, xids=None):
        n, n0 = x.shape[0], self.store.ntotal
        if self.base.ntotal != n0:
            raise ValueError("the base holds %d vectors and the refine store %d: labels are not store positions (set_store)"
                             % (self.base.ntotal, n0))
        ids = np.arange(n0, n0 + n, dtype=np.int64)
        if xids is not None:
            given = xids.cpu().numpy() if _is_torch(xids) else np.asarray(xids)
            if not np.array_equal(given, ids):
                raise ValueError("GpuRefineFlat.add takes the sequential ids ntotal .. ntotal + n - 1 only: a label is a position "
                                 "in the refine store")
        if self._ivf:
            self.base.add(x, ids)
        else:
            self.base.add(x)
        self.store.add(x)

    def set_store(self, vecs):
        """the uncompressed vectors [ntotal][d] of a base whose lists were set, not added: vector i is the one with id i"""
        if vecs.shape[0] != self.base.ntotal:
            raise ValueError("%d vectors for a base of %d" % (vecs.shape[0], self.base.ntotal))
        self.store.reset()
        self.store.add(vecs)

    def reset(self):
        if hasattr(self.base, "reset"):
            self.base.reset()
        else:       # GpuIVFPQ: empty lists
            self.base.set_lists(np.zeros((0, self.base.M), np.uint8), np.zeros((0,), np.int64), np.zeros((self.base.nlist + 1,), np.int64))
        self.store.reset()

    def k_base(self, k):
        """idx_t(k * k_factor), IndexFlat.cpp:224 (one float multiply, truncated)"""
        if not self.k_factor >= 1:
            raise ValueError("k_factor=%r must be >= 1" % (self.k_factor,))
        kb = int(np.float32(k) * np.float32(self.k_factor))
        if kb < k or kb > VLQ_MAX_K:
            raise ValueError("k_base = int(k * k_factor) = %d outside k=%d .. %d" % (kb, k, VLQ_MAX_K))
        return kb

    def _base_search(self, x, k, nprobe, D, I):
        if self._ivf:
            return self.base.search(x, self.nprobe if nprobe is None else nprobe, k, D, I)
        return self.base.search(x, k, D, I)

    def search(self, x, k, nprobe=None, D=None, I=None, store_pairs=False):
        import torch
        if store_pairs:
            raise ValueError("store_pairs labels are (list, offset) pairs, not positions in the refine store")
        if self.base.ntotal != self.store.ntotal:
            raise ValueError("the base holds %d vectors and the refine store %d: the base's labels are not store positions "
                             "(add through GpuRefineFlat, or set_store)" % (self.base.ntotal, self.store.ntotal))
        if k < 1:
            raise ValueError("k=%d must be positive" % k)
        kb = self.k_base(k)
        n = x.shape[0]
        host = not (_is_torch(x) and x.is_cuda)
        xd = torch.as_tensor(np.ascontiguousarray(x, np.float32) if not _is_torch(x) else x).to(self._dev) if host else x
        if host or D is None:
            Dd = torch.empty((n, k), dtype=torch.float32, device=self._dev)
        else:
            Dd = D
        if host or I is None:
            Id = torch.empty((n, k), dtype=torch.int64, device=self._dev)
        else:
            Id = I
        if kb == k:        # the reference's in-place form (IndexFlat.cpp:225-236)
            bD, bI = Dd, Id
        else:
            if self._short is None or self._short[0].shape != (n, kb):
                self._short = (torch.empty((n, kb), dtype=torch.float32, device=self._dev),
                               torch.empty((n, kb), dtype=torch.int64, device=self._dev))
            bD, bI = self._short
        self._base_search(xd, kb, nprobe, bD, bI)
        self.store.refine(xd, bD, bI, k, Dd, Id)      # (synchronises the stream: the rows are complete on return)
        if not host:
            return Dd, Id
        Dh, Ih = Dd.cpu().numpy(), Id.cpu().numpy()
        if D is not None:
            _out_ptr(D, np.float32)
            D[...] = Dh
            Dh = D
        if I is not None:
            _out_ptr(I, np.int64)
            I[...] = Ih
            Ih = I
        return Dh, Ih

    def last_refine_info(self):
        return self.store.last_refine_info()


class GpuVLQ:
    """The fork's vector-and-line-quantization index (include/vlq_line.h):
    GpuIndexIVFPQ(resources, dims, nlist, M, nbits, nedge, nLambda, ...) of
    gpu/GpuIndexIVFPQ.h:60-68 -- construct, load trained state, add, search."""

    def __init__(self, d, nlist, M, nbits, nedge, nlambda, device=0):
        self.d, self.nlist, self.M, self.nbits = d, nlist, M, nbits
        self.nedge, self.nlambda, self.ksub = nedge, nlambda, 1 << nbits
        self._h = C.c_void_p()
        check(lib().vlq_line_create(C.byref(self._h), C.c_int(device), C.c_int(d), C.c_int(nlist),
                                    C.c_int(M), C.c_int(nbits), C.c_int(nedge), C.c_int(nlambda)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().vlq_line_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        check(lib().vlq_line_set_stream(self._h, C.c_void_p(stream_ptr or 0)))

    def set_coarse_centroids(self, c):
        p, _k = _ptr(c, np.float32)
        check(lib().vlq_line_set_coarse_centroids(self._h, p))

    def set_pq_centroids(self, c):
        p, _k = _ptr(c, np.float32)
        check(lib().vlq_line_set_pq_centroids(self._h, p))

    def set_lambda_codebook(self, li):
        p, _k = _ptr(li, np.float32)
        check(lib().vlq_line_set_lambda_codebook(self._h, p))

    def set_float16_tables(self, enable=True):
        """GpuIndexIVFPQConfig::useFloat16LookupTables for the VLQ search (include/vlq_line.h)"""
        check(lib().vlq_line_set_float16_tables(self._h, C.c_int(int(enable))))

    def set_row_mode(self, mode):
        """0 automatic, 1 term-2 rows read from the stored table, 2 rows rebuilt in the scan kernel
        (speed only, identical results; include/vlq_line.h)"""
        check(lib().vlq_line_set_row_mode(self._h, C.c_int(int(mode))))

    def set_scan_parts(self, parts):
        """workgroups per query of the default 16-byte scan (0 = automatic); never changes a result"""
        check(lib().vlq_line_set_scan_parts(self._h, C.c_int(int(parts))))

    def set_graph(self, edge_info, edge_dist):
        pe, _a = _ptr(edge_info, np.int32)
        pd, _b = _ptr(edge_dist, np.float32)
        check(lib().vlq_line_set_graph(self._h, pe, pd))

    def build_graph(self):
        ei = np.empty((self.nlist, self.nedge), np.int32)
        ed = np.empty((self.nlist, self.nedge), np.float32)
        check(lib().vlq_line_build_graph(self._h, ei.ctypes.data_as(C.c_void_p), ed.ctypes.data_as(C.c_void_p)))
        return ei, ed

    def assign(self, x):
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        line = np.empty((n,), np.int32)
        lam = np.empty((n,), np.float32)
        check(lib().vlq_line_assign(self._h, C.c_int64(n), px, line.ctypes.data_as(C.c_void_p),
                                    lam.ctypes.data_as(C.c_void_p)))
        return line, lam

    def residuals(self, x):
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        out = np.empty((n, self.d), np.float32)
        check(lib().vlq_line_residuals(self._h, C.c_int64(n), px, out.ctypes.data_as(C.c_void_p)))
        return out

    def encode(self, x):
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        line = np.empty((n,), np.int32)
        lam = np.empty((n,), np.uint8)
        codes = np.empty((n, self.M), np.uint8)
        check(lib().vlq_line_encode(self._h, C.c_int64(n), px, line.ctypes.data_as(C.c_void_p),
                                    lam.ctypes.data_as(C.c_void_p), codes.ctypes.data_as(C.c_void_p)))
        return line, lam, codes

    def add(self, x, xids=None):
        px, _a = _ptr(x, np.float32)
        pi, _b = _ptr(xids, np.int64)
        check(lib().vlq_line_add(self._h, C.c_int64(x.shape[0]), px, pi))

    def set_lists(self, codes, lambdas, ids, line_offsets):
        pc, _a = _ptr(codes, np.uint8)
        pl, _b = _ptr(lambdas, np.uint8)
        pi, _c = _ptr(ids, np.int64)
        po, _d = _ptr(line_offsets, np.int64)
        check(lib().vlq_line_set_lists(self._h, pc, pl, pi, po))

    @property
    def ntotal(self):
        return int(lib().vlq_line_ntotal(self._h))

    def get_list(self, line):
        n = C.c_int64()
        check(lib().vlq_line_list_length(self._h, C.c_int64(line), C.byref(n)))
        codes = np.empty((n.value, self.M), np.uint8)
        lam = np.empty((n.value,), np.uint8)
        ids = np.empty((n.value,), np.int64)
        check(lib().vlq_line_get_list(self._h, C.c_int64(line), codes.ctypes.data_as(C.c_void_p),
                                      lam.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p)))
        return codes, lam, ids

    def search(self, x, nprobe, w1, k, D=None, I=None, return_lines=False):
        n = x.shape[0]
        px, _a = _ptr(x, np.float32)
        if D is None:
            D = GpuIVFPQ._out(self, None, (n, k), np.float32, x)
        if I is None:
            I = GpuIVFPQ._out(self, None, (n, k), np.int64, x)
        pD, _b = _out_ptr(D, np.float32)
        pI, _c = _out_ptr(I, np.int64)
        lines = np.empty((n, w1), np.int32) if return_lines else None
        pl = lines.ctypes.data_as(C.c_void_p) if return_lines else None
        check(lib().vlq_line_search(self._h, C.c_int64(n), px, C.c_int(nprobe), C.c_int(w1), C.c_int(k),
                                    pD, pI, pl))
        return (D, I, lines) if return_lines else (D, I)

    def stats(self, reset=False):
        nc = C.c_uint64()
        check(lib().vlq_line_stats(self._h, C.byref(nc), C.c_int(int(reset))))
        return nc.value

    def profile(self, enable=True):
        check(lib().vlq_line_profile(self._h, C.c_int(int(enable))))

    def profile_read(self, reset=True):
        """(scan-kernel milliseconds summed over the launches since the last reset, number of launches)"""
        ms, n = C.c_double(), C.c_int64()
        check(lib().vlq_line_profile_read(self._h, C.byref(ms), C.byref(n), C.c_int(int(reset))))
        return ms.value, n.value
