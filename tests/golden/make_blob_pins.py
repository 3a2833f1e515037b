#!/usr/bin/env python3
"""Pins of the packed hx3 parameter blob: tests/golden/blobs/hx3_blob_pins.json.

For every case of CASES: the words of an evaluation handle (gbnf_debug_flow_blob: the host packer) and of a trainer's live blob
after a device re-pack (gbnf_debug_trainer_blob: the live packer) of the same synthetic spec.  Per blob the JSON keeps

    n_words   the word count
    sha256    of the little-endian words with the table-constant words zeroed
    table     the table-constant words in full, as one hex string (8 digits per word, in blob order)

The table-constant words of step s (sb = s * step_words, step_words = (n_words - 64) / K) are word sb + 1 (the log-det constant)
and words sb + 16 .. sb + 335 (the in and out tables: 2 x [slot | p0 | p1 | p2 | p3][4][8]).  Only they go through expf / sqrtf /
logf; every other word is a cast, a float multiply or a double sum and is pinned bit for bit by the hash.

    python tests/golden/make_blob_pins.py [OUT.json]     # (on the GPU) rewrites the JSON from the library as built

tests/test_hip_train.py::test_packed_blobs_match_their_pins rebuilds the same blobs through blobs_of() and compares.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PINS = os.path.join(HERE, "blobs", "hx3_blob_pins.json")
K = 3

# (name, kind, d, h, synth keywords, math modes)
CASES = [
    ("glow_d43_h64_tanh", "glow", 43, 64, {}, ("f16x3", "bf16x6")),
    ("glow_d43_h64_depth0", "glow", 43, 64, {"depth": 0}, ("f16x3",)),
    ("glow_d43_h64_depth2", "glow", 43, 64, {"depth": 2}, ("f16x3",)),
    ("glow_d21_h105_additive", "glow", 21, 105, {"coupling": "additive"}, ("f16x3",)),
    ("glow_d8_h64_relu", "glow", 8, 64, {"act": "relu"}, ("f16x3",)),
    ("glow_d43_h215_tanh", "glow", 43, 215, {}, ("f16x3", "bf16x6")),
    ("realnvp_d21_h105_bn", "realnvp", 21, 105, {}, ("f16x3",)),
    ("realnvp_d6_h30_no_bn", "realnvp", 6, 30, {"batch_norm": False}, ("f16x3",)),
    ("realnvp_d21_h105_mixed", "realnvp", 21, 105, {"coupling_network": "mixed"}, ("f16x3",)),
    ("realnvp_d21_h105_random", "realnvp", 21, 105, {"coupling_network": "random"}, ("f16x3",)),
    ("realnvp_d21_h64_residual1", "realnvp", 21, 64, {"coupling_network": "residual", "depth": 1}, ("f16x3",)),
    ("realnvp_d21_h64_residual2", "realnvp", 21, 64, {"coupling_network": "residual", "depth": 2}, ("f16x3",)),
]


def case_spec(name, math):
    from gbnf_amd import synth
    idx = [c[0] for c in CASES].index(name)
    _, kind, d, h, kw, _ = CASES[idx]
    if kind == "glow":
        spec = synth.synth_glow_spec(d, h, K, seed=4100 + idx, **kw)
    else:
        spec = synth.synth_realnvp_spec(d, h, K, seed=4100 + idx, **kw)
    if name == "glow_d43_h64_tanh" and math == "bf16x6":        # a weight beyond the fp16 range is legal in bf16x6
        spec["steps"][0]["net"]["layers"][0][0][0, 0] = np.float32(3.0e5)
    return spec


def dev_spec(spec, dev):
    """flow spec (numpy) -> device spec (CUDA tensors) for native.NativeTrainer."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    net = lambda n: {"act": n["act"], "layers": [(t(w), t(b)) for w, b in n["layers"]]}
    out = {"kind": spec["kind"], "d": spec["d"], "coupling": spec.get("coupling"), "steps": []}
    for st in spec["steps"]:
        if spec["kind"] == "glow":
            out["steps"].append({"an_bias": t(st["an_bias"]), "an_logs": t(st["an_logs"]), "perm": st["perm"], "net": net(st["net"])})
        else:
            bn = st["bn"]
            out["steps"].append({"flipped": st["flipped"],
                                 "bn": None if bn is None else {**{k: t(bn[k]) for k in ("log_gamma", "beta", "running_mean", "running_var")},
                                                                "eps": bn["eps"]},
                                 "t_net": net(st["t_net"]), "s_net": net(st["s_net"])})
    return out


def _words(fn_name, handle):
    from gbnf_amd import native
    fn = getattr(native.lib(), fn_name)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    fn.restype = C.c_int
    n = C.c_int64()
    native._check(fn(handle, None, C.byref(n)))
    buf = np.zeros(n.value, dtype=np.uint32)
    native._check(fn(handle, buf.ctypes.data_as(C.c_void_p), C.byref(n)))
    return buf


def blobs_of(name, math):
    """{"flow": words, "trainer": words} of one case; a bf16x6 trainer of a geometry without a `safe` line is left out."""
    import torch
    from gbnf_amd import native
    dev = torch.device("cuda:0")
    spec = case_spec(name, math)
    out = {}
    flow = native.NativeFlow(spec, math=math, per_step_activation=name.endswith("_random"))
    out["flow"] = _words("gbnf_debug_flow_blob", flow.handle)
    try:
        tr = native.NativeTrainer(dev_spec(spec, dev), math=math)
    except native.GbnfError:
        if math != "bf16x6":
            raise
        return out
    out["trainer"] = _words("gbnf_debug_trainer_blob", tr.handle)
    return out


def table_mask(n_words):
    assert (n_words - 64) % K == 0
    step_words = (n_words - 64) // K
    m = np.zeros(n_words, dtype=bool)
    for s in range(K):
        m[s * step_words + 1] = True
        m[s * step_words + 16:s * step_words + 336] = True
    return m


def pin_of(words):
    m = table_mask(words.size)
    masked = words.copy()
    masked[m] = 0
    return {"n_words": int(words.size), "sha256": hashlib.sha256(masked.astype("<u4").tobytes()).hexdigest(),
            "table": "".join("%08x" % int(w) for w in words[m])}


def table_words(pin):
    t = pin["table"]
    return np.array([int(t[i:i + 8], 16) for i in range(0, len(t), 8)], dtype=np.uint32)


def all_keys():
    return [(name, math) for name, _, _, _, _, maths in CASES for math in maths]


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    pins = {}
    for name, math in all_keys():
        for which, words in blobs_of(name, math).items():
            pins[f"{name}/{math}/{which}"] = pin_of(words)
            print(f"{name}/{math}/{which}: {words.size} words", flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else PINS
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(pins, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(pins)} pins to {path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
