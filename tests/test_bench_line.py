"""bench.py's result line without a GPU: the compact line of a plain run and of a --full run keep the contract's fields."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

PLAIN = {"metric": "BVH build+traverse throughput", "value": 4712.0, "unit": "Mleaves/s", "n_gpus": 1, "steps": 20, "warmup": 5,
         "ms_per_step": 0.2122, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
         "full": False, "config": {"workload": "w", "leaves_per_gpu": 1000000, "leaves_total": 1000000, "contacts_total": 1760000,
                                   "parallelism": "single GPU"},
         "value_definition": "d", "mcontacts_per_s": 8300.0}
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup")


def test_compact_line_of_a_plain_run_is_the_headline_alone():
    out = bench.compact_line(dict(PLAIN), "bench_detail.json")
    for k in CONTRACT:
        assert out[k] == PLAIN[k], k
    assert out["full"] is False and out["config"] == PLAIN["config"] and out["detail"] == "bench_detail.json"
    assert out["roofline"] is None and out["cpu_baseline"] is None
    assert not {"value_enqueue_only", "north_star_1e7", "configs", "exchange", "dist", "work", "profiled_ms_per_step"} & set(out)
    assert len(json.dumps(out, separators=(",", ":"))) <= 4096


def test_compact_line_of_a_full_run_keeps_the_same_headline():
    roof = {"bound": "hbm", "kernel": "lvt_queue_kernel_count", "achieved": 600.0, "peak": bench.HBM_PEAK_GBS, "unit": "GB/s",
            "frac": 0.075, "traffic": None, "avg_launch_ms": 0.105}
    full = dict(PLAIN, full=True, value_enqueue_only=4750.0, ms_per_step_enqueue_only=0.2105, roofline=roof, cpu_baseline=None,
                work=None, north_star_1e7={"leaves": 10_000_000, "ms_per_step": 1.57, "value": 6356.0, "unit": "Mleaves/s", "roofline": None},
                configs=None, exchange=None, dist=None, kernels={}, profiled_ms_per_step=0.22)
    out = bench.compact_line(full, "bench_detail.json")
    for k in CONTRACT:
        assert out[k] == PLAIN[k], k
    assert out["full"] is True and out["value_enqueue_only"] == 4750.0 and out["roofline"]["kernel"] == "lvt_queue_kernel_count"
    assert out["north_star_1e7"]["leaves"] == 10_000_000
