"""bench.py as a program: a plain run carries the headline alone, --full everything else around the same headline."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

HEADLINE = {"metric": "BVH build+traverse throughput", "unit": "Mleaves/s", "higher_is_better": True, "dtype": "f32", "n_gpus": 1,
            "steps": 3, "warmup": 1}
# what runs of their own measure: in the record of a --full run only
MOVED = ("value_enqueue_only", "ms_per_step_enqueue_only", "roofline", "cpu_baseline", "work", "north_star_1e7", "configs", "exchange",
         "dist", "kernels", "profiled_ms_per_step")


def _bench(tmp_path, tag, *extra):
    detail = tmp_path / f"{tag}.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--n", "200000",
                        "--detail", str(detail), *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), json.load(open(detail))


def test_plain_run_is_the_headline_alone_and_full_adds_the_rest(tmp_path):
    line, detail = _bench(tmp_path, "plain")
    for k, v in HEADLINE.items():
        assert line[k] == v and detail[k] == v, k
    assert line["full"] is False and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(0.2 * 3 / (3 * line["ms_per_step"] * 1e-3), rel=1e-2)  # Mleaves/s from ms_per_step
    assert not [k for k in MOVED if k in detail], "a plain run measured more than its headline"
    assert not [k for k in MOVED if line.get(k) is not None]

    full, full_detail = _bench(tmp_path, "full", "--full", "--no-cpu-baseline", "--no-configs", "--extra-n", "0")
    for k, v in HEADLINE.items():
        assert full[k] == v, k
    assert full["full"] is True and full["value"] > 0
    assert full["config"] == line["config"]  # the same workload, leaves and contacts under the headline
    assert not [k for k in MOVED if k not in full_detail]
    assert full["value_enqueue_only"] > 0 and full["roofline"]["kernel"] and full_detail["kernels"]
