"""What a pre-filter mask costs to build: k_filter_mask_multi against k_filter_count_multi on the same programs, on the device ABI alone.

    python tools/bench_prefilter.py [--docs 10000000] [--reps 20] [--warmup 3]

An index of `docs` documents carries three dictionary-encoded columns (75 / 91 / 8 distinct values, as config 5's year / rating / genre) and Deleted
flags with one document in a thousand set, so that both kernels read the flags.  Programs are `leaf AND leaf` (K = 1: two columns) and a mix over all
three columns (K = 16).  Each call is timed with device events on the stream the kernels run on, recorded around a synchronous call: the programs'
upload (a few hundred bytes), the memset of the counters, ONE kernel launch, the counters' way back.  Reported: the median CALL time over `reps` calls
after `warmup`, and the algorithmic bytes — (columns read x 4 + 1 + K) x docs for the mask kernel (K mask bytes per document written), (columns read x 4 +
1) x docs for the count kernel — over that call time: a call-level rate, a lower bound of what the kernel achieves.  For the kernels' own durations run the
tool under `rocprofv3 --kernel-trace` in a run of its own: per case the launches come in the order of the JSON lines, `warmup + reps` each.  Every case
runs the same programs over the same columns again and again, and part of the columns (40 MB each at 10 M documents) may be served from the 256 MB
Infinity Cache: the rates are not HBM bandwidth figures.  Prints one JSON line per case; needs a GPU (no fallback)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from infidex_amd import load_library  # noqa: E402

NVALS = (75, 91, 8)


class Config(C.Structure):      # infx_config
    _fields_ = [("device", C.c_int32), ("range_docs", C.c_int32), ("max_depth", C.c_int32), ("flags", C.c_int32)]


class Op(C.Structure):          # infx_filter_op
    _fields_ = [("op", C.c_uint32), ("arg", C.c_uint32)]


class Leaf(C.Structure):        # infx_filter_leaf
    _fields_ = [("col", C.c_uint32), ("table_off", C.c_uint32), ("num_values", C.c_uint32), ("reserved", C.c_uint32)]


class Prog(C.Structure):        # infx_filter_prog
    _fields_ = [("ops", C.POINTER(Op)), ("leaves", C.POINTER(Leaf)), ("tables", C.POINTER(C.c_uint32)),
                ("nops", C.c_uint32), ("nleaves", C.c_uint32), ("ntable_words", C.c_uint32), ("reserved", C.c_uint32)]


def p(a, ty):
    return a.ctypes.data_as(C.POINTER(ty))


def make_programs(K, rng, keep):
    """K programs `leaf(colA) AND leaf(colB)`, each leaf a random bitmap over its column's codes; K = 1 reads columns 0 and 1, K = 16 all three."""
    progs = (Prog * K)()
    for k in range(K):
        cols = (0, 1) if K == 1 else ((k % 3), ((k + 1) % 3))
        ops = (Op * 3)(Op(0, 0), Op(0, 1), Op(1, 0))                      # LEAF 0, LEAF 1, AND
        leaves = (Leaf * 2)(); words = []
        for j, c in enumerate(cols):
            nw = (NVALS[c] + 31) // 32
            leaves[j] = Leaf(c, len(words), NVALS[c], 0)
            words += [int(x) for x in rng.integers(0, 1 << 32, nw, dtype=np.uint64)]
        tables = (C.c_uint32 * len(words))(*words)
        keep += [ops, leaves, tables]
        progs[k] = Prog(ops, leaves, tables, 3, 2, len(words), 0)
    return progs, (2 if K == 1 else 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefilter needs a GPU")
    L = load_library()
    L.infx_last_error.restype = C.c_char_p

    def chk(rc):
        if rc:
            raise SystemExit("status %d: %s" % (rc, (L.infx_last_error() or b"").decode()))
    N = a.docs
    rng = np.random.default_rng(11)
    ix = C.c_void_p(); cfg = Config(a.device, 0, 500, 0)
    chk(L.infx_create(C.byref(cfg), C.byref(ix)))
    doc_len = np.ones(N, np.float32); keys = np.arange(N, dtype=np.int64); offs = np.zeros(N + 1, np.uint64); text = np.zeros(1, np.uint16)
    deleted = (rng.integers(0, 1000, N) == 0).astype(np.uint8)
    chk(L.infx_upload_docs(ix, N, p(doc_len, C.c_float), C.c_float(1.0), p(keys, C.c_int64), p(deleted, C.c_uint8), p(offs, C.c_uint64), p(text, C.c_uint16)))
    for c, nv in enumerate(NVALS):
        codes = rng.integers(0, nv, N).astype(np.uint32)
        chk(L.infx_upload_column(ix, c, N, p(codes, C.c_uint32), nv))
    st = C.c_void_p(); chk(L.infx_stream_create(ix, C.byref(st)))
    native = C.c_void_p(); chk(L.infx_stream_native(st, C.byref(native)))
    stream = torch.cuda.ExternalStream(native.value, device=a.device)
    slots = []
    for k in range(16):
        m = C.POINTER(C.c_uint8)(); chk(L.infx_stream_mask_slot(st, k, C.byref(m))); slots.append(m)

    def timed(call):
        ms = []
        for i in range(a.warmup + a.reps):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record(stream); call(); e1.record(stream); e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms)), float(max(ms))
    keep = []
    for K in (1, 16):
        progs, ncol = make_programs(K, rng, keep)
        cnt_m = np.zeros(K, np.uint32); cnt_c = np.zeros(K, np.uint32)
        masks = (C.POINTER(C.c_uint8) * K)(*slots[:K])

        def build_masks():
            chk(L.infx_filter_masks(st, K, progs, masks, p(cnt_m, C.c_uint32)))      # staged ...
            chk(L.infx_stream_wait(st))                                             # ... built and waited for here

        def count():
            chk(L.infx_filter_count_progs(st, K, progs, 1, p(cnt_c, C.c_uint32)))
        for name, call, nbytes in (("k_filter_mask_multi", build_masks, (ncol * 4 + 1 + K) * N), ("k_filter_count_multi", count, (ncol * 4 + 1) * N)):
            med, lo, hi = timed(call)
            print(json.dumps({"kernel": name, "K": K, "docs": N, "columns_read": ncol, "alg_bytes": nbytes, "call_ms_median": round(med, 4), "call_ms_min": round(lo, 4),
                              "call_ms_max": round(hi, 4), "call_GBps_at_median": round(nbytes / med / 1e6, 1), "reps": a.reps}), flush=True)
        assert np.array_equal(cnt_m, cnt_c), (cnt_m, cnt_c)                         # the two kernels agree on every program's count
    L.infx_stream_destroy(st); L.infx_destroy(ix)


if __name__ == "__main__":
    main()
