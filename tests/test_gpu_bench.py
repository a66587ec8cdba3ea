"""bench.py as a plain run: the headline line only (the secondary measurements come with --full), exactly --steps timed
steps, and --dump-outputs writing what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_bench_line_and_dump_outputs(tmp_path):
    out_dir = tmp_path / "dump"
    B = 2048
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--batch", str(B), "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=540)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == 4 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["dtype"] == "f32" and rec["higher_is_better"] is True and rec["unit"] == "codewords/s"
    assert not {"also", "cpu_baseline", "extra", "sim_ber", "end_to_end", "generic_kernel"} & set(rec)
    bits, errs, cnt = (np.load(out_dir / f"{n}.npy") for n in ("decoded_bits_sample", "codeword_bit_errors", "error_counters"))
    assert bits.dtype == np.float32 and bits.shape == (B, 2816) and set(np.unique(bits)) <= {0.0, 1.0}
    assert errs.dtype == np.float32 and errs.shape == (B,)
    assert cnt.dtype == np.float64 and cnt.shape == (4,)
    assert cnt[2] == 4 * B * 2816 and cnt[3] == 4 * B                         # bits and blocks of the 4 timed steps
    assert cnt[0] == 4 * errs.sum() and cnt[1] == 4 * np.count_nonzero(errs)   # every step decodes the same batch
    assert abs(rec["ber"] - cnt[0] / cnt[2]) < 1e-12
