"""Writes tests/golden/boosted_base_state_dicts.json: for the three tiny models of tests/test_boosted_base_host.py, built under that
file's seed, the key order of ``state_dict()`` and a SHA-256 of every tensor.

The recording pins the constructors' draw order, so it is only ever taken from a commit whose constructors are known good -- it was
taken from the last commit in which ``BoostedFlow`` and ``BoostedImageFlow`` each had a constructor of their own.  Running this on a
tree with a changed constructor makes ``test_same_seed_same_model`` pass vacuously: do that only when the draw order is MEANT to change.

    python tests/golden/make_boosted_base_state_dicts.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import torch  # noqa: E402

import test_boosted_base_host as host  # noqa: E402

out = {"seed": host.SEED}
for name, make in host.MODELS.items():
    torch.manual_seed(host.SEED)
    out[name] = host.state_digest(make())
with open(host.RECORDING, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
