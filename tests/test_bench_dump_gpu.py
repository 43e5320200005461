"""bench.py's plain run and `--dump-outputs`: the plain line carries the headline contract and nothing that needs runs of its own
(those are behind --full), and two runs with the same arguments dump the same outputs of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_plain(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "8",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.mark.timeout(700)
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    d, outs = run_plain(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "final_loss"):
        assert k in d, k
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    for k in ("roofline", "cpu_baseline", "decode_tokens_per_s", "other_configs", "fwd_bwd_only"):
        assert k not in d, k
    assert sorted(outs) == ["adam_m", "adam_v", "gpn_loss", "lang_loss", "loss"]
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in outs.values())
    assert sum(v.nbytes for v in outs.values()) <= 64 << 20
    loss, lang, gpn = (outs[k].item() for k in ("loss", "lang_loss", "gpn_loss"))
    assert abs(loss - d["final_loss"]) <= 1e-4 and abs(loss - lang - gpn) <= 1e-5 * abs(loss)
    # same arguments, same inputs, and every step starts from the same weights: the forward is the same to the bit, the gradients (and
    # with them the optimizer's moments) to the rounding of the backward's float-atomic reductions
    _, again = run_plain(tmp_path / "b")
    for k in ("gpn_loss", "lang_loss", "loss"):
        np.testing.assert_allclose(again[k], outs[k], rtol=1e-6)
    for k in ("adam_m", "adam_v"):
        assert again[k].shape == outs[k].shape
        np.testing.assert_allclose(again[k], outs[k], rtol=1e-4, atol=1e-6 * float(np.abs(outs[k]).max()))
