"""The case table of the multi-image tests of the image trainer (tests/test_hip_image_large_batch.py on the device,
tests/test_image_large_batch_host.py on the host): the batch sizes at which the image trainer's launches change shape, each on the
smallest geometry that reaches its regime.  Helper, not a test.

What changes with the batch (restated below from the host code; the host test asserts every regime, the device test anchors the
restatement to the library through the deterministic workspace size):

  weight-gradient slices   wgrad_shape (csrc/gbnf_image_train.hip): blocks of (output tile, input tile) pairs x slices of the
                           (image, strip) items, slices = max(1, min(ceil(items / WGRAD_ITEMS[shape]), 1024 / blocks)); items are dealt
                           item = slice, slice + slices, ...; a strip whose first row lies outside the map is skipped.
  the NLL seed             img_nll_seed_kernel (csrc/gbnf_image_opt.hip): bpc = max(1, min(256 / Cz, ceil(n zH zW / 1024))) workgroups
                           per channel of z, with zH x zW the map proper.
  ActNorm2d init           an_launch_stats: chunks of per_chunk images, at most AN_MAX_CHUNKS = 64, whole groups of 4 (16 x 16 storage)
                           or 16 (8 x 8 storage) images.

Storage: level 0 always lives in 16 x 16 maps, every later level in 8 x 8 maps, whatever the input size (the map proper sits in the
corner); a strip is 4 rows.

name -> (input_size, synth_image_glow_spec keywords, n, seed): synth.synth_image_glow_spec(size, seed=seed, **kw) and
synth.synth_image_batch(n, size, seed=100 + seed); g_z, g_ldj ~ N(0, 1) from RandomState(1000 + seed).

  W1   1 x 32 x 32, h = 256, n = 40    the 1x1 256 -> 256 launch has 16 blocks: capped at 64 slices with 80 wanted, 160 items, slices of 2
                                        or 3 items; the other launches stay uncapped at 27, 40 and 80 slices.  bpc = 10.
  W2   16 x 4 x 4, h = 16, n = 1025     Cz = 64: bpc capped at 4 with 5 wanted, and more rows than one workgroup's 256 threads: the row loop
                                        of the seed strides.  z's map proper is 2 x 2 (n zH zW = 4 n), so the cap needs n > 1024; at the 65
                                        images first proposed for this case bpc is 1.  A 2 x 2 map in 16-row storage: three items of four
                                        lie outside the map; three launches are at the 1024-slice cap (slices of 4 or 5 items), the last
                                        3x3 has 684, and three slices of four see no row of the map.
  W3   1 x 12 x 32, h = 32, n = 32      a 6 x 16 map in 16-row storage.  The 1x1 launches have 64 slices over 128 items: slice y only ever
                                        sees strip y mod 4, half the slices lie outside the map entirely (the last 3x3, 32 slices, too).
  W4   3 x 32 x 32, h = 32, L = 2, n = 24   the CIFAR shape: two levels, Split2d, 8 to 48 slices per launch, bpc = 2, learned top prior.
  W5   1 x 12 x 32, h = 384, n = 16     the > 256-channel two-halves path with 16 images; the 1x1 384 -> 384 launch has 36 blocks: capped
                                        at 28 slices with 32 wanted, 64 items dealt unevenly (2 or 3 per slice).
  A1   1 x 32 x 32, h = 16, K = 2, n = 259  (init only) the 64-chunk cap: 33 chunks of 8 images, the last holding 3 (a wave without an image)
  A2   3 x 32 x 32, h = 32, L = 2, n = 23   (init only) on the 8 x 8 level a group is 16 images: 2 chunks, the last holding 7

Multi-image batches of ReLU nets cannot be kink-free; the host test caps the share of pre-activations inside kink_report's margin at
KINK_SHARE per tensor and shows, by the float32 restatement of the yardstick staying within G_RTOL / 20 of the float64 one, that these
do not move the answer.

Measured on the MI355X (one run; each error as the tests scale it: z by its largest entry, ldj and the nll relative, gradients and g_x
by their tensor's largest entry; the default mode's sums are float atomics, so its last digits move from run to run):
  case  forward z / ldj      gradients, default (g_z = None)   deterministic   step: nll / gradients / top bias, logs   g_x
  W1    3.0e-7 / 1.9e-7      9.4e-7                            1.1e-6          2.9e-8 / 3.0e-7 / 8.8e-8, 1.1e-7          --
  W2    3.6e-7 / 1.8e-7      7.2e-7                            --              9.9e-9 / 6.4e-7 / 1.3e-7, 7.9e-8          --
  W3    2.7e-7 / 1.7e-7      6.9e-7 (7.2e-7)                   5.7e-7          --                                        --
  W4    1.8e-7 / 2.1e-7      3.8e-7 (4.9e-7)                   --              2.6e-10 / 3.1e-7 / 1.5e-7, 1.1e-7         1.4e-6
  W5    2.6e-7 / 2.2e-7      4.1e-7                            3.7e-7          --                                        6.8e-7
  A1    bias / logs 1.2e-7 of max(1, max|ref|)       A2    6.0e-8
All far inside the existing bars (Z_RTOL 2e-5, LL_RTOL 1e-5, G_RTOL 2e-4, BAR 1e-5): no case has a bar of its own, no kernel was changed."""
import functools

import numpy as np

CASES = {
    "W1": ((1, 32, 32), dict(h=256, K=1, L=1), 40, 1),
    "W2": ((16, 4, 4), dict(h=16, K=1, L=1), 1025, 1),
    "W3": ((1, 12, 32), dict(h=32, K=1, L=1), 32, 1),
    "W4": ((3, 32, 32), dict(h=32, K=1, L=2), 24, 1),
    "W5": ((1, 12, 32), dict(h=384, K=1, L=1), 16, 3),
}
# the one-pass ActNorm2d init alone: name -> (input_size, keywords, n); model seed 11, batch seed 3 (tests/image_actnorm_init_cases.py)
INIT_CASES = {
    "A1": ((1, 32, 32), dict(h=16, K=2, L=1), 259),
    "A2": ((3, 32, 32), dict(h=32, K=1, L=2), 23),
}
G_RTOL = 2e-4                  # tests/test_hip_image_train.py (not imported here: that module is a GPU module)
F32_MARGIN = G_RTOL / 20       # the float32 restatement of the yardstick against the float64 one
KINK_SHARE = 2e-4              # ReLU pre-activations within kink_report's margin, per tensor

TR_R = 4                       # rows of a strip
WGRAD_ITEMS = (6, 4, 2)        # least items of a slice: first 3x3, last 3x3, 1x1
WGRAD_MAX_WORKGROUPS = 1024
OPT_MAX_PARTIALS = 256         # csrc/gbnf_opt.h
SEED_ENTRIES = 1024            # entries of a channel one seed workgroup takes before a second is added (4 x 256 threads)
AN_MAX_CHUNKS = 64


def _cdiv(a, b):
    return -(-a // b)


# ---- the host formulas, restated --------------------------------------------------------------------------------------------------
def levels(size, L):
    """[(C, H, Hv, Wv)] per level: channels after the squeeze, rows (= columns) of the storage, the map proper
    (gbnf_image_trainer_create)."""
    C, Hv, Wv = size
    H, out = 32, []
    for l in range(L):
        C, H, Hv, Wv = C * 4, max(H // 2, 8), Hv // 2, Wv // 2
        out.append((C, H, Hv, Wv))
        if l < L - 1:
            C //= 2
    return out


def convolutions(size, kw):
    """[(what, level, cout, cin, ks)] of every weight-gradient launch of a backward, in table order: per step its 1x1 mix and the
    convolutions of its net, per level but the last its Split2d prior."""
    L, K, h, depth = kw["L"], kw["K"], kw["h"], kw.get("depth", 1)
    affine = kw.get("coupling", "affine") == "affine"
    out = []
    for l, (C, _, _, _) in enumerate(levels(size, L)):
        c1, c2 = C // 2, C - C // 2
        for k in range(K):
            out.append((f"level {l} step {k} mix", l, C, C, 1))
            out.append((f"level {l} step {k} conv 0", l, h, c1, 3))
            out += [(f"level {l} step {k} conv {q}", l, h, h, 1) for q in range(1, depth + 1)]
            out.append((f"level {l} step {k} conv {depth + 1}", l, 2 * c2 if affine else c2, h, 3))
        if l < L - 1:
            out.append((f"level {l} split", l, C, C // 2, 3))
    return out


def wgrad_shape(cout, cin, ks, H, n):
    """wgrad_shape (csrc/gbnf_image_train.hip) -> (blocks, slices, slices wanted, items)."""
    items = n * (H // TR_R)
    OT, IT, NP = _cdiv(cout, 16), _cdiv(cin, 16), 2 if ks == 3 else 4
    obt = 4 if OT >= 4 else (2 if OT >= 2 else 1)
    ibt = min(4 * NP // obt, 8, IT)
    blocks = _cdiv(OT, obt) * _cdiv(IT, ibt)
    min_items = WGRAD_ITEMS[2 if ks == 1 else (0 if OT >= IT else 1)]
    wanted = _cdiv(items, min_items)
    return blocks, max(1, min(wanted, WGRAD_MAX_WORKGROUPS // blocks)), wanted, items


def launch_table(name):
    """Per weight-gradient launch of a case: dict(what, cout, cin, ks, blocks, slices, wanted, capped, items, per_slice = (fewest,
    most) items of a slice, empty = the slices that hold no item inside the map, region = floats of its (dW', db'))."""
    size, kw, n, _ = CASES[name]
    lv = levels(size, kw["L"])
    rows = []
    for what, l, cout, cin, ks in convolutions(size, kw):
        _, H, Hv, _ = lv[l]
        blocks, slices, wanted, items = wgrad_shape(cout, cin, ks, H, n)
        strips = H // TR_R
        held = [list(range(y, items, slices)) for y in range(slices)]
        inside = [[i for i in h if (i % strips) * TR_R < Hv] for h in held]
        rows.append(dict(what=what, cout=cout, cin=cin, ks=ks, blocks=blocks, slices=slices, wanted=wanted, capped=wanted > slices,
                         items=items, per_slice=(min(map(len, held)), max(map(len, held))),
                         empty=[y for y in range(slices) if not inside[y]], region=cout * cin * ks * ks + cout))
    return rows


def seed_bpc(name):
    """img_nll_seed_kernel's grid -> (Cz, bpc, bpc wanted)."""
    size, kw, n, _ = CASES[name]
    Cz, _, Hv, Wv = levels(size, kw["L"])[-1]
    wanted = _cdiv(n * Hv * Wv, SEED_ENTRIES)
    return Cz, max(1, min(OPT_MAX_PARTIALS // Cz, wanted)), wanted


def an_chunks(H, n):
    """an_launch_stats on H x H storage -> (per_chunk, chunks, group)."""
    group = 4 * (256 // (H * H))
    want = min(AN_MAX_CHUNKS, _cdiv(n, group))
    per_chunk = _cdiv(_cdiv(n, want), group) * group
    return per_chunk, _cdiv(n, per_chunk), group


def det_extra_bytes(name):
    """gbnf_image_trainer_workspace_bytes in deterministic mode minus the default mode's (train_space): the log-det slots of one
    launch -- n x strips x 4 waves on the level with the most strips; a log-det-carrying convolution has at most 128 output channels,
    which conv_o_split leaves at one workgroup per strip -- and the partials of the largest weight-gradient launch, each rounded
    up to 64 floats."""
    size, kw, n, _ = CASES[name]
    up = lambda v: _cdiv(v, 64) * 64
    ldj = n * 4 * max(H // TR_R for _, H, _, _ in levels(size, kw["L"]))
    return 4 * (up(ldj) + up(max(r["slices"] * r["region"] for r in launch_table(name))))


# ---- inputs and yardsticks (float64, computed once, shared, left unchanged) -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_case(name):
    """-> (spec, x, noise, g_z, g_ldj) of a listed case."""
    from gbnf_amd import synth
    size, kw, n, seed = CASES[name]
    spec = synth.synth_image_glow_spec(size, seed=seed, **kw)
    x, noise = synth.synth_image_batch(n, size, seed=100 + seed)
    Cz, _, Hv, Wv = levels(size, kw["L"])[-1]
    rng = np.random.RandomState(1000 + seed)
    g_z = rng.standard_normal((n, Cz, Hv, Wv)).astype(np.float32)
    g_ldj = rng.standard_normal(n).astype(np.float32)
    return spec, x, noise, g_z, g_ldj


@functools.lru_cache(maxsize=None)
def grads(name, with_gz=True, dtype_name="float64"):
    """image_grad_oracle.grads of a case -> (out, {path: gradient})."""
    import torch
    import image_grad_oracle as igo
    spec, x, noise, g_z, g_ldj = make_case(name)
    out, ref = igo.grads(spec, x, noise, g_z if with_gz else None, g_ldj, dtype=getattr(torch, dtype_name))
    assert tuple(out["z"].shape) == g_z.shape
    return out, ref


@functools.lru_cache(maxsize=None)
def input_grad(name):
    """float64 d (sum g_z z + sum g_ldj ldj_noperm) / dx of a case."""
    import torch
    import image_grad_oracle as igo
    spec, x, noise, g_z, g_ldj = make_case(name)
    xl = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    out = igo.forward(spec, igo.leaf_params(spec), xl, noise)
    ((torch.as_tensor(g_z, dtype=torch.float64) * out["z"]).sum() + (torch.as_tensor(g_ldj, dtype=torch.float64) * out["ldj_noperm"]).sum()).backward()
    return xl.grad.numpy()


@functools.lru_cache(maxsize=None)
def step_yardstick(name):
    """image_step_oracle.step_yardstick of a case -> (nll, {path: gradient of the nll})."""
    import image_step_oracle as iso
    spec, x, noise, _, _ = make_case(name)
    return iso.step_yardstick(spec, x, noise)


def worst_grad_error(got, ref):
    """The measure of test_hip_image_train._check_grads: max over the tensors of max|got - ref| / max(max|ref|, 1e-3)."""
    assert set(got) == set(ref)
    return max(float(np.abs(np.asarray(got[p], dtype=np.float64) - ref[p]).max()) / max(float(np.abs(ref[p]).max()), 1e-3) for p in ref)


def make_init(name):
    """-> (spec with every ActNorm2d zeroed, x, noise) of an INIT_CASES entry."""
    import image_actnorm_init_cases as aic
    from gbnf_amd import synth
    size, kw, n = INIT_CASES[name]
    spec = aic.zeroed(synth.synth_image_glow_spec(size, seed=aic.MODEL_SEED, **kw))
    return (spec, *synth.synth_image_batch(n, size, seed=aic.BATCH_SEED))


@functools.lru_cache(maxsize=None)
def init_oracle(name, dtype_name="float64"):
    """oracle.image_actnorm_init of an INIT_CASES entry -> [(bias, logs)] in module order."""
    import torch
    from oracle import gbnf_oracle as oracle
    spec, x, noise = make_init(name)
    return oracle.image_actnorm_init(spec, x, noise, dtype=getattr(torch, dtype_name))
