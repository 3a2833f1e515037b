"""GPU: a plain `bench.py` run times exactly the steps it is given and, with --dump-outputs, writes G of its last timed step --
the batch the oracle computes here from the same seeds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_err

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_steps_G(tmp_path):
    from gbnf_amd import synth
    from oracle import gbnf_oracle as oracle
    steps, group = 40, 32          # one full group and a partial one of 8: the last timed step is batch 7 of the second group
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "4",
                          "--prewarm", "0", "--dump-outputs", str(tmp_path)],
                         stdout=subprocess.PIPE, text=True, timeout=600, check=True).stdout
    line = json.loads(out.strip().splitlines()[-1])
    assert line["steps"] == steps and line["config"]["group"] == group and line["timing"]["repetitions"] == 1
    assert line["ms_per_step"] == pytest.approx(line["timing"]["elapsed_ms_median"] / steps)
    assert line["cpu_baseline"] is None and "legs_summary" not in line and line["full_record"] is None
    G = np.load(tmp_path / "G.npy")
    assert G.dtype == np.float32 and G.shape == (4096,)
    # bench.py's workload: miniboone_glow C = 8, weights from seed 1, batch j of a group from seed 100 + j (batch 0: seed 0)
    specs = synth.synth_boosted_specs("glow", 8, 43, 215, 5, seed=1)
    x = synth.synth_batch(4096, 43, seed=100 + (steps - 1) % group)
    rho = np.maximum(1.0 / np.power(2.0, np.arange(8)), 0.05).astype(np.float32)
    _, G_ref = oracle.mixture_log_prob(specs, rho, x)
    assert rel_err(G, G_ref) < 1e-5
