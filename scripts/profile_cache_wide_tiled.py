"""cache_topk_wide_tiled against cache_topk_wide and torch.matmul + torch.max
on one MI355X: the sweep behind profiles/cache_topk_wide_tiled.md.

Per shape every op is warmed, then the ops are timed alternately, one call
between two device events each, and the median and spread per op are printed
as one JSON line. Results are compared on the same inputs before timing.
--variant names further builds of the extension (the same source with
-DAIGW_WIDE_TILED_TI=...) to time next to it."""

import argparse
import importlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

# public MI355X peaks the floors are computed against
HBM_BYTES_PER_S = 8.0e12
MFMA_FLOPS = {"bf16": 2.5e15, "fp8": 5.0e15}


def time_alternately(ops, warm, reps):
    """{name: [ms, ...]}: one event-timed call of each op per round."""
    for fn in ops.values():
        for _ in range(warm):
            fn()
    times = {name: [] for name in ops}
    for _ in range(reps):
        for name, fn in ops.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[768, 1024, 1536, 2048])
    ap.add_argument("--queries", type=int, nargs="+", default=[37, 128, 256])
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sweeps", type=int, default=2)
    ap.add_argument("--variant", action="append", default=[],
                    help="module name of another build of the extension")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"

    import aigw_hip

    variants = {name: importlib.import_module(name) for name in args.variant}
    g = torch.Generator(device="cuda").manual_seed(11)
    row_scope = torch.randint(1, 9, (args.rows,), generator=g, device="cuda")
    row_expiry = torch.where(torch.arange(args.rows, device="cuda") % 8 == 7, 0, 0x7FFFFFFF).int()
    for sweep in range(args.sweeps):
        for dim in args.dims:
            rows = torch.nn.functional.normalize(
                torch.randn(args.rows, dim, generator=g, device="cuda"), dim=1)
            picks = torch.randint(0, args.rows, (256,), generator=g, device="cuda")
            noise = torch.randn(256, dim, generator=g, device="cuda") * (0.04 / dim**0.5)
            qf = torch.nn.functional.normalize(rows[picks] + noise, dim=1)
            for dtype_name, dtype in (("bf16", torch.bfloat16), ("fp8", torch.float8_e4m3fn)):
                index = rows.to(dtype)
                for n_q in args.queries:
                    q = qf[:n_q].to(dtype).contiguous()
                    q_scope = (torch.arange(n_q, device="cuda") % 9).long()
                    for scoped in (False, True):
                        tags = (row_scope, row_expiry, q_scope, 1) if scoped else ()
                        fp8 = dtype_name == "fp8"
                        per_pass = aigw_hip.cache_wide_queries_per_pass(dim, fp8, scoped)
                        ops = {
                            "tiled": lambda: aigw_hip.cache_topk_wide_tiled(index, q, *tags),
                            "wide": lambda: aigw_hip.cache_topk_wide(index, q, *tags),
                        }
                        for name, mod in variants.items():
                            ops[name] = (lambda m: lambda: m.cache_topk_wide_tiled(
                                index, q, *tags))(mod)
                        if not fp8 and not scoped:
                            ops["matmul_max"] = lambda: torch.max(
                                torch.matmul(q, index.T), dim=1)
                        # results first: the same row for every query, and the
                        # scores' largest difference in fp32
                        t_hi, t_idx = ops["tiled"]()
                        w_hi, w_idx = ops["wide"]()
                        same = {"rows_differ_from_wide": int((t_idx != w_idx).sum()),
                                "hi_differ_from_wide": int((t_hi != w_hi).sum())}
                        for name in variants:
                            v_hi, v_idx = ops[name]()
                            same[name + "_rows_differ"] = int((v_idx != t_idx).sum())
                            same[name + "_hi_differ"] = int((v_hi != t_hi).sum())
                        if "matmul_max" in ops:
                            same["rows_differ_from_matmul"] = int(
                                (ops["matmul_max"]()[1] != t_idx).sum())
                        times = time_alternately(ops, args.warm, args.reps)
                        flops = 2.0 * args.rows * n_q * dim
                        byts = args.rows * dim * (1 if fp8 else 2)
                        floor_hbm = byts / HBM_BYTES_PER_S * 1e3
                        floor_mfma = flops / MFMA_FLOPS[dtype_name] * 1e3
                        print(json.dumps({
                            "sweep": sweep, "dtype": dtype_name, "dim": dim, "queries": n_q,
                            "scoped": scoped, "wide_passes": -(-n_q // per_pass),
                            "ms": {k: round(statistics.median(v), 4) for k, v in times.items()},
                            "spread": {k: round((max(v) - min(v)) / statistics.median(v), 3)
                                       for k, v in times.items()},
                            "floor_ms": round(max(floor_hbm, floor_mfma), 4),
                            "floor": "hbm" if floor_hbm >= floor_mfma else "mfma",
                            **same,
                        }), flush=True)
                del index
            del rows


if __name__ == "__main__":
    main()
