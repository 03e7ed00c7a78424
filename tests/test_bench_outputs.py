"""bench.py output contract: the result line of a plain run, and
--dump-outputs writing the same arrays on every run with the same
arguments (so two builds can be compared output for output)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WAVES, BATCH = 3, 2, 4


def _run_bench(out_dir, *extra, steps=STEPS):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO
    proc = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--steps", str(steps), "--warmup", "1", "--waves", str(WAVES),
         "--batch", str(BATCH), "--workers", "1",
         "--dump-outputs", str(out_dir), *extra],
        env=env, capture_output=True, timeout=170, cwd=REPO,
    )
    assert proc.returncode == 0, proc.stderr.decode()[-2000:]
    lines = [l for l in proc.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.timeout(180)
def test_dump_outputs_repeatable(tmp_path):
    out_a = _run_bench(tmp_path / "a")
    out_b = _run_bench(tmp_path / "b", "--full")

    for out in (out_a, out_b):
        for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                    "ms_per_step"):
            assert key in out, key
        assert out["steps"] == STEPS
        assert out["ms_per_step"] > 0
        # value is the request rate of exactly STEPS timed steps
        per_step = BATCH * WAVES
        # ms_per_step is printed to 0.001 ms and value to 0.01 req/s: the
        # bound is those two roundings, nothing else
        rel = 0.0005 / out["ms_per_step"] + 0.005 / out["value"]
        assert out["value"] == pytest.approx(
            per_step / (out["ms_per_step"] / 1000.0), rel=1.01 * rel)
    # the direct-latency baseline is a --full measurement
    assert out_a["config"]["p50_added_latency_ms"] is None
    assert out_b["config"]["p50_added_latency_ms"] is not None

    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["accounting_per_step.npy", "response_lengths.npy",
                     "responses.npy"]
    assert sorted(os.listdir(tmp_path / "b")) == names
    for n in names:
        a = np.load(tmp_path / "a" / n)
        b = np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64
        assert np.array_equal(a, b), n

    resp = np.load(tmp_path / "a" / "responses.npy")
    lens = np.load(tmp_path / "a" / "response_lengths.npy")
    assert resp.shape[0] == BATCH and lens.tolist() == [resp.shape[1]] * BATCH
    body = json.loads(bytes(resp[0].astype(np.uint8)))
    assert body["object"] == "chat.completion"
    assert body["usage"]["prompt_tokens"] == 4096

    import bench

    acct = dict(zip(bench.DUMP_COUNTERS,
                    np.load(tmp_path / "a" / "accounting_per_step.npy")))
    assert acct["requests"] == acct["responses_2xx"] == BATCH * WAVES
    assert acct["total_tokens"] == BATCH * WAVES * (4096 + 16)


@pytest.mark.gpu
@pytest.mark.timeout(180)
def test_dump_gpu_tokens_match_oracle(tmp_path):
    """The gpu_tokens column is the one dumped figure the HIP admission
    kernels produce: per step it must be the CPU BPE oracle's count for
    the benchmark payload times the requests of a step."""
    import bench
    from aigw.ops.bpe_ref import BPERef, make_merges

    out = _run_bench(tmp_path / "g", steps=2)
    assert out["config"]["gpu_token_accounting"] is True
    assert out["config"]["front"] == "fast"

    # chat text extraction appends one newline per collected value
    text = b"".join(m["content"].encode() + b"\n"
                    for m in bench.build_payload(4096)["messages"])
    per_request = len(BPERef(make_merges(32768, 1355)).encode_batch([text])[0])
    assert per_request > 4096

    acct = dict(zip(bench.DUMP_COUNTERS,
                    np.load(tmp_path / "g" / "accounting_per_step.npy")))
    assert acct["requests"] == BATCH * WAVES
    assert acct["gpu_tokens"] == per_request * BATCH * WAVES
