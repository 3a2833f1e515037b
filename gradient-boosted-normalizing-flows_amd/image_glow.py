"""Host mirror of the reference's IMAGE Boosted-Glow (BASELINE.json configs[3]) on the density-evaluation path.

``BoostedFlow(args)`` returns a ``BoostedImageFlow`` when ``args.input_size`` has more than one dimension.  The module
tree reproduces the reference's parameter names and shapes (tests/golden/state_dict_layout.json: ``image_*``), so a
reference checkpoint loads with ``load_state_dict``; every call that computes goes to ``libgbnf_hip.so``
(``native.NativeImageFlow``) -- there is no eager / CPU path.

Reference anchors: Glow (models/glow.py:12-110), FlowNet image branch (:192-252), FlowStep (:264-342), ActNorm2d /
Conv2d / Conv2dZeros / Permute2d / Split2d / SqueezeLayer / InvertibleConv1x1 (models/layers.py:548-796), BoostedFlow
(models/boosted_flow.py), the image likelihood ll = log_normal_diag(z, z_mu, z_var) + logdet (image_experiment.py:227).
Class conditioning (``args.y_condition``: a per-image prior from ``project_ycond`` and the class head ``project_class``,
models/glow.py:36-39, 79-82, 105-106) runs in the library too (gbnf_image_ycond.hip); the boosted wrapper passes ``y_onehot`` on to the
component, which the reference's ``BoostedFlow.encode`` forgets.  Not on the path: learned dequantisation flows.  In train mode with gradients enabled a component's forward runs on the
live parameters and is differentiable (``native.NativeImageTrainer``: HIP forward and backward, exact f32; ``torch.optim`` on the
resulting ``.grad`` is the supported step).  An un-initialised model (fresh from the constructor)
is initialised from data with ``BoostedImageFlow.initialize_actnorms(x)`` -- what the reference's first training-mode forward
does (models/layers.py:473-486) -- or by loading a trained checkpoint / ``set_actnorm_init``.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn

from . import native
from .boosted_base import BoostedMixtureBase, image_deterministic_from, image_eval_deterministic_from


def _no_eager(*a, **k):
    raise RuntimeError("image layers are evaluated by the HIP kernels, not module by module")


class ActNorm2d(nn.Module):
    def __init__(self, num_features, scale=1.0):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(1, num_features, 1, 1))
        self.logs = nn.Parameter(torch.zeros(1, num_features, 1, 1))
        self.num_features, self.scale, self.inited, self.image_input = num_features, scale, False, True


class Conv2d(nn.Module):
    """models/layers.py:577-606: conv without bias + ActNorm2d."""

    def __init__(self, in_dim, out_dim, kernel_size=(3, 3), weight_std=0.05):
        super().__init__()
        pad = ((kernel_size[0] - 1) // 2, (kernel_size[1] - 1) // 2)
        self.conv = nn.Conv2d(in_dim, out_dim, kernel_size, 1, pad, bias=False)
        self.conv.weight.data.normal_(mean=0.0, std=weight_std)
        self.actnorm = ActNorm2d(out_dim)
        self.do_actnorm = True
    forward = _no_eager


class Conv2dZeros(nn.Module):
    """models/layers.py:609-630."""

    def __init__(self, in_dim, out_dim, logscale_factor=3):
        super().__init__()
        self.conv = nn.Conv2d(in_dim, out_dim, (3, 3), 1, (1, 1))
        self.conv.weight.data.zero_()
        self.conv.bias.data.zero_()
        self.logscale_factor = logscale_factor
        self.logs = nn.Parameter(torch.zeros(out_dim, 1, 1))
    forward = _no_eager


class LinearZeros(nn.Module):
    """models/layers.py:560-574: (x W^T + b) exp(3 logs), zero at construction."""

    def __init__(self, in_dim, out_dim, logscale_factor=3):
        super().__init__()
        self.linear = nn.Linear(in_dim, out_dim)
        self.linear.weight.data.zero_()
        self.linear.bias.data.zero_()
        self.logscale_factor = logscale_factor
        self.logs = nn.Parameter(torch.zeros(out_dim))

    def forward(self, sample):          # (tiny, and only on the autograd path of a class-conditional component)
        return self.linear(sample) * torch.exp(self.logs * self.logscale_factor)


class ConvNet(nn.Module):
    """models/layers.py:304-317."""

    def __init__(self, in_dim, out_dim, hidden_dim, num_layers=1):
        super().__init__()
        layers = [Conv2d(in_dim, hidden_dim)]
        for _ in range(num_layers):
            layers += [nn.ReLU(), Conv2d(hidden_dim, hidden_dim, kernel_size=(1, 1))]
        layers += [nn.ReLU(), Conv2dZeros(hidden_dim, out_dim)]
        self.network = nn.Sequential(*layers)
    forward = _no_eager


class Permute2d(nn.Module):
    """models/layers.py:633-680: indices are plain attributes (not in state_dict)."""

    def __init__(self, num_dim, shuffle):
        super().__init__()
        self.num_dim = num_dim
        self.indices = torch.arange(num_dim - 1, -1, -1, dtype=torch.long)
        if shuffle:
            self.indices = self.indices[torch.randperm(num_dim)]

    def __setattr__(self, name, value):
        if name == "indices":        # every (re)assignment gets a new serial number: the handle keys use it
            object.__setattr__(self, "indices_serial", getattr(self, "indices_serial", 0) + 1)
        super().__setattr__(name, value)

    def set_indices(self, indices):
        idx = torch.as_tensor(np.asarray(indices), dtype=torch.long).clone()
        if idx.shape != (self.num_dim,) or sorted(idx.tolist()) != list(range(self.num_dim)):
            raise ValueError("indices must be a permutation of range(num_dim)")
        self.indices = idx


class InvertibleConv1x1(nn.Module):
    """models/layers.py:722-749: either the plain (C,C) weight or its LU factors (p, sign_s buffers; lower, log_s, upper)."""

    def __init__(self, num_dim, LU_decomposed):
        super().__init__()
        w_init = torch.linalg.qr(torch.randn(num_dim, num_dim))[0]
        self.LU_decomposed = LU_decomposed
        self.w_shape = [num_dim, num_dim]
        if not LU_decomposed:
            self.weight = nn.Parameter(w_init)
        else:
            p, lower, upper = torch.linalg.lu(w_init)
            s = torch.diag(upper)
            self.register_buffer("p", p)
            self.register_buffer("sign_s", torch.sign(s))
            self.lower = nn.Parameter(lower)
            self.log_s = nn.Parameter(torch.log(torch.abs(s)))
            self.upper = nn.Parameter(torch.triu(upper, 1))

    def composed_weight(self):
        """What get_weight returns in the forward direction (models/layers.py:751-776), as float64 numpy."""
        if not self.LU_decomposed:
            return self.weight.detach().double().cpu().numpy()
        n = self.w_shape[0]
        l_mask = torch.tril(torch.ones(n, n, dtype=torch.float64), -1)
        lower = self.lower.detach().double().cpu() * l_mask + torch.eye(n, dtype=torch.float64)
        u = self.upper.detach().double().cpu() * l_mask.t() + torch.diag(
            self.sign_s.double().cpu() * torch.exp(self.log_s.detach().double().cpu()))
        return (self.p.double().cpu() @ (lower @ u)).numpy()

    def composed_weight_tensor(self):
        """The same matrix as a differentiable float32 tensor on the parameters' device (the training path's 1x1 weight): the chain
        from its gradient to lower / upper / log_s is torch autograd on C x C."""
        if not self.LU_decomposed:
            return self.weight
        n = self.w_shape[0]
        l_mask = torch.tril(torch.ones(n, n, dtype=self.lower.dtype, device=self.lower.device), -1)
        lower = self.lower * l_mask + torch.eye(n, dtype=self.lower.dtype, device=self.lower.device)
        u = self.upper * l_mask.t() + torch.diag(self.sign_s * torch.exp(self.log_s))
        return self.p @ (lower @ u)

    def composed_log_det(self):
        """log|det| of that matrix, differentiable: sum(log_s) for the LU form, slogdet otherwise (models/layers.py:756, 790; C x C in
        float64 on the parameters' device)."""
        if self.LU_decomposed:
            return self.log_s.sum()
        return torch.linalg.slogdet(self.weight.double())[1].to(self.weight.dtype)


class FlowStep(nn.Module):
    def __init__(self, in_dim, hidden_dim, actnorm_scale, flow_permutation, flow_coupling, LU_decomposed, args):
        super().__init__()
        self.image_input, self.flow_coupling = True, flow_coupling
        self.actnorm = ActNorm2d(in_dim, actnorm_scale)
        if flow_permutation == "invconv":
            self.invconv = InvertibleConv1x1(in_dim, LU_decomposed)
        elif flow_permutation == "shuffle":
            self.shuffle = Permute2d(in_dim, shuffle=True)
        else:
            self.reverse = Permute2d(in_dim, shuffle=False)
        cin, cout = in_dim // 2, in_dim - in_dim // 2
        if flow_coupling not in ("additive", "affine"):
            raise ValueError(f"flow_coupling={flow_coupling!r}")
        self.block = ConvNet(cin, cout if flow_coupling == "additive" else 2 * cout, hidden_dim,
                             args.coupling_network_depth)


class SqueezeLayer(nn.Module):
    def __init__(self, factor):
        super().__init__()
        self.factor = factor


class Split2d(nn.Module):
    def __init__(self, in_dim):
        super().__init__()
        self.conv = Conv2dZeros(in_dim // 2, in_dim)


class FlowNet(nn.Module):
    """models/glow.py:192-233, image branch."""

    def __init__(self, args):
        super().__init__()
        self.image_input, self.K, self.L = True, args.num_flows, args.num_blocks
        self.layers = nn.ModuleList()
        self.output_shapes = []
        C, H, W = args.input_size
        for i in range(self.L):
            C, H, W = C * 4, H // 2, W // 2
            self.layers.append(SqueezeLayer(2))
            self.output_shapes.append([-1, C, H, W])
            for _ in range(self.K):
                self.layers.append(FlowStep(C, args.h_size, args.actnorm_scale, args.flow_permutation, args.flow_coupling,
                                            args.LU_decomposed, args))
            self.output_shapes.append([-1, C, H, W])
            if i < self.L - 1:
                self.layers.append(Split2d(C))
                self.output_shapes.append([-1, C // 2, H, W])
                C = C // 2


class ImageGlow(nn.Module):
    """models/glow.py:12-58 for image input."""

    def __init__(self, args):
        super().__init__()
        if getattr(args, "num_dequant_blocks", 0) > 0:
            raise NotImplementedError("learned dequantisation flows are not on the supported path")
        self.learn_top, self.y_condition, self.y_classes = bool(args.learn_top), bool(getattr(args, "y_condition", False)), args.y_classes
        if self.y_condition and not 1 <= int(self.y_classes) <= 256:
            raise NotImplementedError(f"y_condition with y_classes={self.y_classes}: the class-conditional kernels take 1 to 256 classes")
        self.sample_size, self.image_input = args.sample_size, True
        self.input_size = [int(v) for v in args.input_size]
        self.hidden = int(args.h_size)
        self.flow = FlowNet(args)
        Cz, Hz, Wz = self.flow.output_shapes[-1][1:]
        if self.learn_top:
            self.learn_top_fn = Conv2dZeros(Cz * 2, Cz * 2)
        if self.y_condition:
            self.project_ycond = LinearZeros(int(self.y_classes), 2 * Cz)
            self.project_class = LinearZeros(Cz, int(self.y_classes))
        self.register_buffer("prior_h", torch.zeros([1, Cz * 2, Hz, Wz]))
        self.register_buffer("bounds", torch.tensor([0.9], dtype=torch.float32))
        self.dequant_flows = None

    def _actnorms(self):
        return [m for m in self.modules() if isinstance(m, ActNorm2d)]

    def set_actnorm_init(self):
        """models/glow.py:181-187."""
        for m in self._actnorms():
            m.inited = True


def actnorm_skip_flags(glow):
    """The ``skip`` argument of native.NativeImageTrainer.actnorm_init for an ImageGlow: one flag per ActNorm2d in module order (per
    FlowStep its own, then the one behind each Conv2d of its coupling net), true = initialised already, leave it alone."""
    return [bool(m.inited) for m in glow._actnorms()]


def _np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32))


def _conv_spec(m):
    zeros = isinstance(m, Conv2dZeros)
    return {"w": _np(m.conv.weight), "b": _np(m.conv.bias) if m.conv.bias is not None else None,
            "an_bias": None if zeros else _np(m.actnorm.bias).reshape(-1),
            "an_logs": None if zeros else _np(m.actnorm.logs).reshape(-1),
            "logs": _np(m.logs).reshape(-1) if zeros else None}


def image_spec_from_glow_module(glow):
    """ImageGlow (this mirror; the reference's module has the same attributes) -> image flow spec (synth.py)."""
    if not all(bool(m.inited) for m in glow._actnorms()):
        raise ValueError("ActNorm not initialised (models/layers.py:473-475 raises in eval mode too)")
    levels, steps = [], []
    coupling = None
    for layer in glow.flow.layers:
        if isinstance(layer, FlowStep):
            st = {"an_bias": _np(layer.actnorm.bias).reshape(-1), "an_logs": _np(layer.actnorm.logs).reshape(-1),
                  "perm_w": None, "perm": None}
            if hasattr(layer, "invconv"):
                st["perm_w"] = layer.invconv.composed_weight().astype(np.float32)
            else:
                pm = layer.shuffle if hasattr(layer, "shuffle") else layer.reverse
                st["perm"] = np.asarray(pm.indices.cpu().numpy(), dtype=np.int64)
            st["convs"] = [_conv_spec(m) for m in layer.block.network if not isinstance(m, nn.ReLU)]
            coupling = layer.flow_coupling
            steps.append(st)
        elif isinstance(layer, Split2d):
            levels.append({"steps": steps, "split": _conv_spec(layer.conv)})
            steps = []
    levels.append({"steps": steps, "split": None})
    spec = {"kind": "glow_image", "input_size": list(glow.input_size), "hidden": glow.hidden, "coupling": coupling,
            "bounds": float(glow.bounds.item()), "levels": levels,
            "learn_top": _conv_spec(glow.learn_top_fn) if glow.learn_top else None}
    if getattr(glow, "y_condition", False):          # (the key is absent from an unconditional component's spec)
        spec["ycond"] = _ycond_spec(glow)
    return spec


def _ycond_spec(glow):
    """project_ycond / project_class of a class-conditional ImageGlow -> the spec's "ycond" entry (native.NativeImageFlow.set_ycond)."""
    pc, pk = glow.project_ycond, glow.project_class
    return {"cond_w": _np(pc.linear.weight), "cond_b": _np(pc.linear.bias), "cond_logs": _np(pc.logs),
            "class_w": _np(pk.linear.weight), "class_b": _np(pk.linear.bias), "class_logs": _np(pk.logs)}


def _put(dst, src):
    with torch.no_grad():
        dst.copy_(torch.as_tensor(np.asarray(src), dtype=dst.dtype).reshape(dst.shape).to(dst.device))


def _load_conv(m, c):
    _put(m.conv.weight, c["w"])
    if c["b"] is not None:
        _put(m.conv.bias, c["b"])
    if c["an_bias"] is not None:
        _put(m.actnorm.bias, c["an_bias"])
        _put(m.actnorm.logs, c["an_logs"])
        m.actnorm.inited = True
    if c["logs"] is not None:
        _put(m.logs, c["logs"])


def load_image_spec(glow, spec):
    """Install an image flow spec's numbers into an ImageGlow (plain-weight invconv or Permute2d components)."""
    steps = [st for lv in spec["levels"] for st in lv["steps"]]
    splits = [lv["split"] for lv in spec["levels"] if lv["split"] is not None]
    si = pi = 0
    for layer in glow.flow.layers:
        if isinstance(layer, FlowStep):
            st = steps[si]
            si += 1
            _put(layer.actnorm.bias, st["an_bias"])
            _put(layer.actnorm.logs, st["an_logs"])
            layer.actnorm.inited = True
            if hasattr(layer, "invconv"):
                if layer.invconv.LU_decomposed:
                    raise NotImplementedError("load_image_spec installs a composed matrix: build the module with LU_decomposed=False")
                _put(layer.invconv.weight, st["perm_w"])
            else:
                (layer.shuffle if hasattr(layer, "shuffle") else layer.reverse).set_indices(st["perm"])
            convs = [m for m in layer.block.network if not isinstance(m, nn.ReLU)]
            if len(convs) != len(st["convs"]):
                raise ValueError("coupling network depth mismatch")
            for m, c in zip(convs, st["convs"]):
                _load_conv(m, c)
        elif isinstance(layer, Split2d):
            _load_conv(layer.conv, splits[pi])
            pi += 1
    if spec["learn_top"] is not None:
        _load_conv(glow.learn_top_fn, spec["learn_top"])
    yc = spec.get("ycond")
    if (yc is not None) != bool(getattr(glow, "y_condition", False)):
        raise ValueError("the spec and the module disagree about y_condition")
    if yc is not None:
        if yc.get("class_w") is None:
            raise ValueError("a module's class-conditional component has a class head: the spec's ycond entry needs class_w / class_b / class_logs")
        for lin, pre in ((glow.project_ycond, "cond"), (glow.project_class, "class")):
            _put(lin.linear.weight, yc[pre + "_w"])
            _put(lin.linear.bias, yc[pre + "_b"])
            _put(lin.logs, yc[pre + "_logs"])


class _ImageFlowFunction(torch.autograd.Function):
    """(z, ldj) of one component on its live parameters (native.NativeImageTrainer); the backward calls the library.  ``tensors``: the
    bound parameters in the order of ``paths`` (for an LU step the composed 1x1 matrix: autograd carries its gradient on to lower /
    upper / log_s), saved for autograd's in-place-modification check only."""

    @staticmethod
    def forward(ctx, trainer, x, noise, paths, *tensors):
        z, ldj, trace = trainer.forward(x, noise)
        ctx.trainer, ctx.trace, ctx.paths = trainer, trace, paths
        ctx.save_for_backward(*tensors)
        return z, ldj

    @staticmethod
    def backward(ctx, g_z, g_ldj):
        tensors = ctx.saved_tensors              # (raises if an optimiser stepped between forward and backward)
        _, views = ctx.trainer.backward(ctx.trace, g_z.contiguous().float(), g_ldj.contiguous().float())
        return (None, None, None, None) + tuple(views[p].view_as(t) for p, t in zip(ctx.paths, tensors))


class _ImageFlowInputGradFunction(torch.autograd.Function):
    """``_ImageFlowFunction`` whose backward also returns the gradient with respect to x (gbnf_image_trainer_backward_x): the
    ``input_grad=True`` form of ``component_forward``.  ``noise`` is held fixed."""

    @staticmethod
    def forward(ctx, trainer, x, noise, paths, *tensors):
        x = x.detach().contiguous()
        z, ldj, trace = trainer.forward(x, noise)
        ctx.trainer, ctx.trace, ctx.paths, ctx.x, ctx.noise = trainer, trace, paths, x, noise
        ctx.save_for_backward(*tensors)
        return z, ldj

    @staticmethod
    def backward(ctx, g_z, g_ldj):
        tensors = ctx.saved_tensors
        g_x, _, views = ctx.trainer.backward_x(ctx.trace, ctx.x, ctx.noise, g_z.contiguous().float(), g_ldj.contiguous().float(),
                                               want_grads=True)
        return (None, g_x, None, None) + tuple(views[p].view_as(t) for p, t in zip(ctx.paths, tensors))


class BoostedImageFlow(BoostedMixtureBase):
    """models/boosted_flow.py:BoostedFlow for image components: density evaluation, z -> x, and (train mode, gradients enabled) the
    differentiable forward of one component."""

    _CACHES = ("_tensor_cache",)

    def __init__(self, args):
        if args.component_type != "glow":
            raise NotImplementedError("image components are Glow (models/boosted_flow.py:44-50 builds nothing else for images)")
        super().__init__(args)
        # Two flags.  `deterministic` (BoostedFlow: args.deterministic / env GBNF_DETERMINISTIC) was defined when only the tabular
        # trainer had ordered sums: an image module that carries it builds and evaluates as ever and its first TRAINING call is
        # refused (native_trainer) -- behaviour the suite pins.  `image_deterministic` (args.image_deterministic / env
        # GBNF_IMAGE_DETERMINISTIC) asks for the image trainer's own ordered path (gbnf_image_trainer_set_deterministic) and is
        # applied to every trainer native_trainer() hands out; with it set the refusal does not fire.  (One flag would do once
        # the refusal is no longer expected of `deterministic` alone.)
        # A third, `image_eval_deterministic` (args.image_eval_deterministic / env GBNF_IMAGE_EVAL_DETERMINISTIC), asks for the
        # EVALUATION handles' ordered log-det sums (gbnf_image_flow_set_deterministic) and is applied to every handle native_flow()
        # hands out: component_forward (eval), component_log_prob, log_prob, forward(y_onehot=...), update_rho, _rho_gradients and
        # the fixed-mixture term of training_step(fixed=...) then repeat bit for bit.  It reads neither of the other two.
        self.image_deterministic = image_deterministic_from(args)
        self.image_eval_deterministic = image_eval_deterministic_from(args)
        self.flows.extend(ImageGlow(args) for _ in range(self.num_components))
        dev = getattr(args, "device", None)
        if dev is not None:
            self.to(dev)

    def _component_tensors(self, c):
        """(parameters, buffers, Permute2d modules, ActNorm modules) of component c, collected once: walking the module
        tree per call costs about as much as a small launch.  `_apply` (.to / .cuda / .float) drops the cache."""
        cache = self.__dict__.setdefault("_tensor_cache", {})
        if c not in cache:
            flow = self.flows[c]
            cache[c] = (list(flow.parameters()), list(flow.buffers()),
                        [m for m in flow.modules() if isinstance(m, Permute2d)], list(flow._actnorms()))
        return cache[c]

    def native_flow(self, c):
        flow = self.flows[c]
        params, buffers, perms, actnorms = self._component_tensors(c)
        key = tuple(int(t._version) for t in params) + tuple(int(t._version) for t in buffers) + \
            tuple(t.data_ptr() for t in params) + \
            tuple((m.indices_serial, int(m.indices._version)) for m in perms) + \
            tuple(bool(m.inited) for m in actnorms)
        cached = self._handles.get(c)
        if cached is None or cached[0] != key:
            self._handles[c] = (key, native.NativeImageFlow(image_spec_from_glow_module(flow)))
        handle = self._handles[c][1]
        want = bool(getattr(self, "image_eval_deterministic", False))
        if getattr(handle, "_eval_deterministic", False) != want:      # (also a cached handle after the module's flag changed)
            handle.deterministic = want
            handle._eval_deterministic = want
        return handle

    def _y(self, c, y_onehot, n=None):
        """``y_onehot`` as component c's kernels take it: (n, y_classes) contiguous float32 on the device; None for an unconditional
        component (which ignores the argument, as the reference does).  A class-conditional one refuses None (the reference asserts)."""
        flow = self.flows[c]
        if not flow.y_condition:
            return None
        if y_onehot is None:
            raise ValueError("this model is class-conditional (y_condition): y_onehot is required")
        self._require_device(y_onehot)
        if y_onehot.dim() != 2 or y_onehot.shape[1] != int(flow.y_classes) or (n is not None and y_onehot.shape[0] != n):
            raise ValueError(f"y_onehot must be ({'n' if n is None else n}, {int(flow.y_classes)}), got {tuple(y_onehot.shape)}")
        return y_onehot.contiguous().float()

    def _recording(self, c):
        """Train mode with gradients enabled: the component's forward is recorded for autograd."""
        return self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self._component_tensors(c)[0])

    def native_trainer(self, c):
        """(native.NativeImageTrainer bound to component c's live parameter storage, bindings), cached like ``native_flow`` and keyed
        on the tensors' addresses (not their versions: an optimiser's in-place update needs no new trainer).  bindings: one
        (path, parameter | InvertibleConv1x1 module, persistent composed matrix | None, pixels of the level) per bound tensor.

        Two flags, for a reason of history: ``deterministic`` alone is refused here, as it was while the image trainer had no
        ordered path; ``image_deterministic`` switches every trainer handed out (cached ones included) to the ordered sums."""
        if self.deterministic and not self.image_deterministic:
            raise native.GbnfError("deterministic mode is on, but the image trainer's ordered path is asked for by a flag of its own: "
                                   "set image_deterministic (args.image_deterministic / env GBNF_IMAGE_DETERMINISTIC) as well "
                                   "(without it the weight gradients and log-det sums are added with unordered float atomics)")
        trainer, bind = self._native_trainer(c)
        if trainer._deterministic != bool(self.image_deterministic):     # (also a cached trainer after the module's flag changed)
            trainer.deterministic = bool(self.image_deterministic)
        return trainer, bind

    def _native_trainer(self, c, allow_uninit=False):
        """``allow_uninit``: for ``initialize_actnorms(fused=True)`` only, which binds the un-initialised layers in order to write them."""
        flow = self.flows[c]
        params, buffers, perms, actnorms = self._component_tensors(c)
        if not allow_uninit and not all(bool(m.inited) for m in actnorms):
            raise ValueError("ActNorm not initialised: call initialize_actnorms(x) (or load a checkpoint) before training")
        key = tuple(t.data_ptr() for t in params) + tuple(t.data_ptr() for t in buffers) + \
            tuple((m.indices_serial, int(m.indices._version)) for m in perms)
        cached = self._trainers.get(c)
        if cached is not None and cached[0] == key:
            return cached[1], cached[2]
        bind = []

        def conv(m, path):
            zeros = isinstance(m, Conv2dZeros)
            out = {"w": m.conv.weight, "b": m.conv.bias, "an_bias": None if zeros else m.actnorm.bias,
                   "an_logs": None if zeros else m.actnorm.logs, "logs": m.logs if zeros else None}
            for k in native.NativeImageTrainer.CONV_KEYS:
                if out[k] is not None:
                    bind.append((path + (k,), out[k], None))
                    out[k] = out[k].detach()
            return out

        levels, steps, coupling = [], [], None
        for layer in flow.flow.layers:
            l, k = len(levels), len(steps)
            if isinstance(layer, FlowStep):
                path = ("levels", l, "steps", k)
                st = {"an_bias": layer.actnorm.bias.detach(), "an_logs": layer.actnorm.logs.detach(), "perm_w": None, "perm": None}
                bind.append((path + ("an_bias",), layer.actnorm.bias, None))
                bind.append((path + ("an_logs",), layer.actnorm.logs, None))
                if hasattr(layer, "invconv"):
                    inv = layer.invconv
                    # LU: one persistent (C, C) tensor per step, the composed matrix is copied in before each forward.  So is a plain
                    # weight that is not row-major in memory (the constructor's QR factor is column-major): the library binds rows.
                    if inv.LU_decomposed or not inv.weight.is_contiguous():
                        st["perm_w"] = torch.empty(tuple(inv.w_shape), dtype=torch.float32, device=actnorms[0].bias.device)
                        bind.append((path + ("perm_w",), inv, st["perm_w"]))
                    else:
                        st["perm_w"] = inv.weight.detach()
                        bind.append((path + ("perm_w",), inv, None))
                else:
                    pm = layer.shuffle if hasattr(layer, "shuffle") else layer.reverse
                    st["perm"] = np.asarray(pm.indices.cpu().numpy(), dtype=np.int64)
                st["convs"] = [conv(m, path + ("convs", q))
                               for q, m in enumerate(mm for mm in layer.block.network if not isinstance(mm, nn.ReLU))]
                coupling = layer.flow_coupling
                steps.append(st)
            elif isinstance(layer, Split2d):
                levels.append({"steps": steps, "split": conv(layer.conv, ("levels", l, "split"))})
                steps = []
        levels.append({"steps": steps, "split": None})
        dev_spec = {"kind": "glow_image", "input_size": list(flow.input_size), "hidden": flow.hidden, "coupling": coupling,
                    "bounds": float(flow.bounds.item()), "levels": levels, "learn_top": None}
        with torch.cuda.device(params[0].device):
            trainer = native.NativeImageTrainer(dev_spec)
        self._trainers[c] = (key, trainer, bind)
        return trainer, bind

    @staticmethod
    def _row_major_1x1(flow):
        """Contiguous float32 storage for every 1x1 tensor and buffer of the component (``_step_trainer``'s docstring)."""
        for layer in flow.flow.layers:
            inv = getattr(layer, "invconv", None)
            for p in ([] if inv is None else ([inv.lower, inv.upper, inv.log_s, inv.p, inv.sign_s] if inv.LU_decomposed else [inv.weight])):
                if not p.is_contiguous() or p.dtype != torch.float32:
                    p.data = p.data.float().contiguous()

    def _step_trainer(self, c):
        """``native_trainer(c)`` for the fused step, which updates the bound tensors themselves: (trainer, bindings) with the live LU
        factors and ``learn_top_fn`` bound on top (once per trainer object).  A 1x1 tensor or buffer that is not row-major in memory
        (the constructor's QR / LU factors are column-major) gets contiguous storage first.  Only ``.data`` is re-set: the Parameter
        object, and so any torch optimiser holding it, is unchanged, and the library binds the module's own storage, never a copy."""
        flow = self.flows[c]
        self._row_major_1x1(flow)
        trainer, bind = self.native_trainer(c)
        if not getattr(trainer, "step_bound", False):
            with torch.cuda.device(trainer.device):
                for path, obj, _ in bind:
                    if isinstance(obj, InvertibleConv1x1) and obj.LU_decomposed:
                        trainer.bind_lu(path[1], path[3], obj.p.detach(), obj.sign_s.detach(), obj.lower.detach(), obj.upper.detach(),
                                        obj.log_s.detach())
                if flow.learn_top:
                    top = flow.learn_top_fn
                    trainer.bind_top(top.conv.weight.detach(), top.conv.bias.detach(), top.logs.detach())
                if flow.y_condition:
                    pc, pk = flow.project_ycond, flow.project_class
                    for t in (pc.linear.weight, pc.linear.bias, pc.logs, pk.linear.weight, pk.linear.bias, pk.logs):
                        if not t.is_contiguous() or t.dtype != torch.float32:
                            t.data = t.data.float().contiguous()
                    trainer.bind_ycond(pc.linear.weight.detach(), pc.linear.bias.detach(), pc.logs.detach(), pk.linear.weight.detach(),
                                       pk.linear.bias.detach(), pk.logs.detach())
            trainer.step_bound = True
        return trainer, bind

    def _step_names(self, c, bind=None):
        """{path in the trainer's step layout: parameter name within flows[c]} of every tensor the fused step updates."""
        flow = self.flows[c]
        if bind is None:
            _, bind = self._step_trainer(c)
        ids = {id(p): name for name, p in flow.named_parameters()}
        names = {}
        for path, obj, _ in bind:
            if not isinstance(obj, InvertibleConv1x1):
                names[path] = ids[id(obj)]
            elif obj.LU_decomposed:
                for key in ("lower", "upper", "log_s"):
                    names[path[:-1] + (key,)] = ids[id(getattr(obj, key))]
            else:
                names[path] = ids[id(obj.weight)]
        if flow.learn_top:
            top = flow.learn_top_fn
            names.update({("learn_top", "w"): ids[id(top.conv.weight)], ("learn_top", "b"): ids[id(top.conv.bias)],
                          ("learn_top", "logs"): ids[id(top.logs)]})
        if flow.y_condition:
            pc, pk = flow.project_ycond, flow.project_class
            for key, t in zip(native.NativeImageTrainer.YCOND_KEYS,
                              (pc.linear.weight, pc.linear.bias, pc.logs, pk.linear.weight, pk.linear.bias, pk.logs)):
                names[("ycond", key)] = ids[id(t)]
        return names

    def step_parameters(self, c):
        """The component's ``nn.Parameter`` objects in the order of the trainer's step layout (None for a reserved region): the
        ``params`` argument of ``native.OptState.load_from`` / ``store_to`` against a ``torch.optim`` optimiser on them."""
        trainer, bind = self._step_trainer(int(c))
        names, by_name = self._step_names(int(c), bind), dict(self.flows[int(c)].named_parameters())
        return [None if t is None else by_name[names[path]] for (path, _, _), t in zip(trainer._step_regions, trainer.params)]

    def opt_state(self, c, optimizer="adamw", trainer=None):
        """The ``native.OptState`` ``training_step`` keeps for component c (created on first use; another ``optimizer`` kind or a
        re-bound component starts a new one)."""
        if trainer is None:
            trainer, _ = self._step_trainer(int(c))
        states = self.__dict__.setdefault("_opt_states", {})
        st = states.get(int(c))
        if st is None or st.kind != optimizer or st.grad_floats != trainer.step_grad_floats or st.exp_avg_device != trainer.device:
            st = states[int(c)] = native.OptState(trainer, optimizer)
        return st

    def training_step(self, x, *, lr, weight_decay=0.0, max_grad_norm=0.0, optimizer="adamw", betas=(0.9, 0.999), eps=1e-8,
                      noise=None, bits_per_dim=True, want_grads=False, fixed=None, g_floor=-10.0, y_onehot=None, y_weight=0.01):
        """The body of one iteration of the reference's image training loop (image_experiment.py:378-419) for ``self.component`` in one
        library call (gbnf_image_trainer_nll_step): the loss ``mean(-(log_normal_diag(z, z_mu, z_var) + logdet))`` -- divided by
        ``ln 2 * C*H*W`` with ``bits_per_dim`` (:227-229) --, ``loss.backward()``, ``clip_grad_norm_`` (``max_grad_norm`` > 0) and the
        step of ``optim.AdamW`` / ``optim.SGD`` ("adamw" | "sgd") on the component's parameters, in place: the LU factors of the 1x1
        convolutions and ``learn_top_fn`` included.  ``lr`` is per call (schedulers stay with the caller).  ``noise``: the U(0,1)
        dequantisation noise (drawn when None).  Returns 0-dim DEVICE tensors (nothing is read back): ``nll`` (nats), ``bpd``,
        ``grad_norm`` (of the scaled loss: what the reference clips), ``clip_coef``; with ``want_grads`` also ``grads``: {parameter name
        within ``flows[c]``: view of the unclipped gradient}.  The optimiser state is kept per component (``self.opt_state(c)``).  No
        ``p.grad`` is written.

        ``fixed``: the fixed-mixture term of the boosted image loss (:247-261, :398-402).  It has no gradient with respect to the trained
        component, so the update is the same with and without it; with it the step is gbnf_image_boosted_nll_step, which also evaluates
        the fixed component on the same ``(x, noise)`` and returns, besides the keys above, ``G_nll`` = mean(-max(ll_G, ``g_floor``))
        (the reference's G_MAX_LOSS is -10), ``boosted_nll`` = nll - G_nll (what the reference reports and feeds its plateau scheduler)
        and ``boosted_bpd`` as 0-dim device tensors, and ``fixed_component`` (int).  ``fixed=None`` (default): no such term, today's
        return.  ``fixed="sample"``: the reference's draw, ``_sample_component('-c' if all_trained else '1:c-1')`` (a host read of
        ``rho`` with more than one candidate); for the FIRST component this is the trained component itself, as in the reference, whose
        evaluation handle is then re-packed every step because its parameters move: ``fixed=None`` is recommended there.  ``fixed=int``:
        that component.

        ``y_onehot`` (n, y_classes), required by a class-conditional model: the loss gains ``y_weight`` * mean cross-entropy of the
        class head against argmax(y_onehot) (image_experiment.py:231-239, the cross_entropy branch; the reference's y_weight is 0.01),
        the prior is per image, and the six tensors of ``project_ycond`` / ``project_class`` are updated too
        (gbnf_image_trainer_nll_step_y).  The result gains ``loss_classes`` (the mean cross-entropy, unweighted) and ``class_correct``
        (rows whose largest logit is at argmax y).  A ``fixed`` component is evaluated with the same ``y_onehot``."""
        self._require_device(x)
        if x.requires_grad:
            raise NotImplementedError("the image training path has no gradient with respect to x")
        c = int(self.component)
        flow = self.flows[c]
        fc = None
        if isinstance(fixed, str):
            if fixed != "sample":
                raise ValueError(f"fixed must be None, 'sample' or a component index, got {fixed!r}")
            fc = self._sample_component("-c" if self.all_trained else "1:c-1")
        elif fixed is not None:
            fc = int(fixed)
            if isinstance(fixed, bool) or not 0 <= fc < self.num_components:
                raise ValueError(f"fixed={fixed!r} is no component of this model (0 .. {self.num_components - 1})")
        x = x.contiguous().float()
        noise = torch.rand_like(x) if noise is None else noise.contiguous().float()
        y = self._y(c, y_onehot, x.shape[0])
        if y is not None:
            if fc is not None and not self.flows[fc].y_condition:
                raise ValueError("the fixed component of a class-conditional step must be class-conditional too")
            hyper_y = dict(y=y, y_weight=float(y_weight))
        else:
            hyper_y = {}
        with torch.cuda.device(x.device):
            trainer, bind = self._step_trainer(c)
            state = self.opt_state(c, optimizer, trainer)
            per_dim = 1.0 / (float(np.log(2.0)) * float(np.prod(flow.input_size)))
            hyper = dict(loss_scale=per_dim if bits_per_dim else 1.0, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                         betas=betas, eps=eps)
            if fixed is None:
                stats, flat = trainer.nll_step(x, noise, state, **hyper, **hyper_y)
            else:
                stats, flat = trainer.boosted_nll_step(self.native_flow(fc), x, noise, state, g_floor=g_floor, **hyper, **hyper_y)
        # the kernels wrote the parameters behind autograd's back: move their version counters (host only, no launch) so that the
        # packed evaluation copy keyed on them (native_flow) is rebuilt
        torch.autograd.graph.increment_version(self._component_tensors(c)[0])
        out = {"nll": stats[0], "bpd": stats[0] * per_dim, "grad_norm": stats[1], "clip_coef": stats[2]}
        g = 8 if y is not None else 4                    # (the class-conditional calls keep the G term behind the class statistics)
        if y is not None:
            out.update({"loss_classes": stats[4], "class_correct": stats[5]})
        if fc is not None:
            out.update({"G_nll": stats[g], "boosted_nll": stats[g + 1], "boosted_bpd": stats[g + 1] * per_dim, "fixed_component": fc})
        if want_grads:
            views = trainer.step_views(flat)
            out["grads"] = {name: views[path] for path, name in self._step_names(c, bind).items()}
        return out

    def _component_forward_train(self, x, c, noise, y=None, input_grad=False):
        """Differentiable (z, z_mu, z_var, ldj, y_logits) of component c on its live parameters (models/glow.py:92-110).  y_logits is
        None for an unconditional component; a class-conditional one forms its per-image prior and its logits from the live
        ``project_ycond`` / ``project_class`` with torch ops on (n, 2Cz) and (n, Y) tensors, so the reference's own
        ``loss.backward()`` loop reaches all six tensors.  ``input_grad``: the backward also returns the gradient with respect to x."""
        if x.requires_grad and not input_grad:
            raise NotImplementedError("the image training path has no gradient with respect to x")
        if input_grad and x.dtype != torch.float32:
            raise ValueError("input_grad needs a float32 x")
        flow = self.flows[c]
        trainer, bind = self.native_trainer(c)
        paths, tensors, log_dets, plain = [], [], [], {}
        for path, obj, persistent in bind:
            if isinstance(obj, InvertibleConv1x1):
                w = obj.composed_weight_tensor()
                if persistent is not None:
                    with torch.no_grad():
                        persistent.copy_(w)
                if obj.LU_decomposed:
                    log_dets.append(trainer.level_pixels[path[1]] * obj.composed_log_det())
                else:                                    # plain matrices: ONE batched float64 slogdet per level, on the device
                    plain.setdefault(path[1], []).append(w)
                obj = w
            paths.append(path)
            tensors.append(obj)
        with torch.cuda.device(x.device):
            fn = _ImageFlowInputGradFunction if input_grad else _ImageFlowFunction
            z, ldj = fn.apply(trainer, x, noise, tuple(paths), *tensors)
        for l, ws in plain.items():
            log_dets.append(trainer.level_pixels[l] * torch.linalg.slogdet(torch.stack(ws).double())[1].sum().to(z.dtype))
        if log_dets:                                     # the 1x1 matrices' own log-determinants: closed form on C x C
            ldj = ldj + torch.stack(log_dets).sum()
        Cz = z.shape[1]
        if flow.learn_top:                               # Conv2dZeros of a zero input: bias * exp(3 logs); its weight gets a zero gradient
            top = flow.learn_top_fn
            h = top.conv.bias * torch.exp(top.logs.view(-1) * top.logscale_factor) + 0.0 * top.conv.weight.sum()
            z_mu, z_var = h[:Cz].view(1, -1, 1, 1).expand(z.shape), h[Cz:].view(1, -1, 1, 1).expand(z.shape)
        else:
            h = None
            z_mu = z_var = torch.zeros((), dtype=z.dtype, device=z.device).expand(z.shape)
        if not flow.y_condition:
            return z, z_mu, z_var, ldj, None
        yp = flow.project_ycond(y)                       # (n, 2Cz), models/glow.py:79-82
        hy = yp if h is None else h.view(1, -1) + yp
        z_mu, z_var = hy[:, :Cz].view(-1, Cz, 1, 1).expand(z.shape), hy[:, Cz:].view(-1, Cz, 1, 1).expand(z.shape)
        return z, z_mu, z_var, ldj, flow.project_class(z.mean(2).mean(2))

    def component_forward(self, x, c, noise=None, want_z=True, y_onehot=None, input_grad=False):
        """x (N,C,H,W) in [0,1] -> z, ldj, ll of component c.  ``noise``: the U(0,1) dequantisation noise
        (models/glow.py:135); drawn on the device when None.  In train mode with gradients enabled: the differentiable
        (z, z_mu, z_var, ldj, y_logits) of ``forward`` on the live parameters instead.  A class-conditional component needs
        ``y_onehot`` (n, y_classes) and returns the reference's five values in evaluation mode too:
        (z, z_mu, z_var, ldj, y_logits) with the (n,Cz,1,1) priors expanded as views -- its ll under that prior is
        ``component_log_prob``'s.  ``input_grad`` (a recorded call only): an ``x`` that requires grad gets its gradient from
        ``backward()`` as well (the noise held fixed); without the keyword such an x is refused as ever."""
        self._require_device(x)
        y = self._y(int(c), y_onehot, x.shape[0])
        if self._recording(int(c)):
            xx = x if x.requires_grad else x.contiguous().float()
            nn_ = torch.rand_like(xx) if noise is None else noise.contiguous().float()
            return self._component_forward_train(xx, int(c), nn_, y, input_grad=bool(input_grad) and x.requires_grad)
        x = x.contiguous().float()
        if noise is None:
            noise = torch.rand_like(x)
        with torch.cuda.device(x.device):
            handle = self.native_flow(int(c))
            if y is None:
                return handle.forward(x, noise.contiguous().float(), want_z=want_z)
            z, ldj, _, logits = handle.forward(x, noise.contiguous().float(), want_z=True, y=y)
            mu, lv, _ = handle.prior_y(y)
        cz = z.shape[1]
        return z, mu.view(-1, cz, 1, 1).expand(z.shape), lv.view(-1, cz, 1, 1).expand(z.shape), ldj, logits

    def numerics_status(self, n_used=None, direction="forward"):
        """State of the image path's numerics protocol over the first n_used components (no synchronisation), with the keys of
        BoostedFlow.numerics_status: dict(math_mode, demoted, checks, worst_rel_err, tolerance).  ``checks`` / ``worst_rel_err`` are
        the on-data checks of the direction asked for (gbnf_image_flow_repair_counts, gbnf_image_flow_inverse_check_counts), summed /
        the largest over the components; math_mode and demoted belong to the handles (a failed check of either direction sends a
        handle to exact f32): "f32" as soon as one component runs there."""
        inverse = native.check_direction(direction) == "inverse"
        n_used = self._n_used(n_used, "all")
        checks, worst, demoted, mode, tol = 0, 0.0, False, None, 0.0
        for c in range(n_used):
            h = self.native_flow(c)
            st = h.numerics()
            if inverse:
                k = h.inverse_check_counts()
                checks, worst = checks + k["data_checks"], max(worst, k["worst_rel_err"])
            else:
                k = h.repair_counts()
                checks, worst = checks + k["data_checks"], max(worst, k["worst_check_rel_err"])
            demoted = demoted or bool(st.demoted)
            mode = int(st.math_mode) if mode is None else min(mode, int(st.math_mode))
            tol = float(st.tolerance)
        return {"math_mode": native.MATH_NAME[mode], "demoted": demoted, "checks": int(checks), "worst_rel_err": float(worst),
                "tolerance": tol}

    def _prior_on(self, handle, device):
        prior = handle.__dict__.get("_prior_dev")            # (mean, logvar) of the top prior on the device, per handle
        if prior is None or prior[0].device != device:
            mu, lv = handle.prior()
            prior = (torch.from_numpy(mu).to(device).view(1, -1, 1, 1), torch.from_numpy(lv).to(device).view(1, -1, 1, 1))
            handle.__dict__["_prior_dev"] = prior
        return prior

    def decode(self, z, y_onehot=None, temperature=1.0, components="c", eps=None, e=None):
        """models/boosted_flow.py:208-218 -> Glow.decode (models/glow.py:112-123) of one component (the reference's own
        BoostedFlow.decode dies on a misspelt keyword; the component-level decode is the parity target,
        fixtures g16_*).  z None: ``sample_size`` draws from the top prior, z = Normal(z_mu, exp(z_var) * temperature) as the
        reference writes it.  ``eps``: the standard-normal draws of the Split2d levels (native.NativeImageFlow.inverse).
        A class-conditional component with z None draws ``y_onehot.shape[0]`` images, row i from the prior of ``y_onehot[i]``
        (gbnf_image_flow_prior_y; ``e``: the standard-normal draws behind the top latents, (n,) + z_shape, drawn when None) -- the
        reference's Glow.decode(z=None, y_onehot=y) dies on ``data.shape[0]`` of a None (models/glow.py:82)."""
        c = self._sample_component(components) if isinstance(components, str) else int(components)
        handle = self.native_flow(c)
        temperature = 1.0 if temperature is None else float(temperature)
        if z is None and self.flows[c].y_condition:
            y = self._y(c, y_onehot)
            with torch.cuda.device(y.device):
                if e is None:
                    e = torch.randn((y.shape[0],) + tuple(handle.z_shape), device=y.device, dtype=torch.float32)
                z = handle.prior_y(y, e.contiguous().float(), temperature, want_prior=False)[2]
        elif z is None:
            dev = self.rho.device
            mu, lv = self._prior_on(handle, dev)
            n = int(self.flows[c].sample_size)
            z = mu + torch.exp(lv) * temperature * torch.randn((n,) + tuple(handle.z_shape), device=dev)
        if not z.is_cuda:
            raise native.GbnfError("z must live on the MI355X (cuda) device: this module has no CPU path")
        with torch.cuda.device(z.device):
            return handle.inverse(z.contiguous().float(), eps, temperature)

    # ---- the component as the bijection it is: x -> (z, eps) -> x (gbnf_image_flow_encode / gbnf_image_flow_inverse) on the evaluation
    # handles, no gradients.  ``noise`` None: no dequantisation noise is added (u = 255 x / 256), so the calls are deterministic.
    def _latent_args(self, x, components, noise):
        self._require_device(x)
        c = self._sample_component(components) if isinstance(components, str) else int(components)
        x = x.contiguous().float()
        if noise is not None:
            self._require_device(noise)
            noise = noise.contiguous().float()
        return c, x, noise

    @torch.no_grad()
    def encode_latent(self, x, components, noise=None):
        """x (n,C,H,W) in [0,1] -> (z, eps) of one component: the top latent and the list of standardised halves its Split2d levels
        drop (native.NativeImageFlow.encode), the form ``decode(z, eps=eps, temperature=1.0, components=c)`` takes back."""
        c, x, noise = self._latent_args(x, components, noise)
        with torch.cuda.device(x.device):
            z, eps, _, _ = self.native_flow(c).encode(x, noise)
        return z, eps

    @torch.no_grad()
    def reconstruct(self, x, components, noise=None):
        """decode(encode_latent(x)) at temperature 1: the dequantised input u = (255 x + noise) / 256 to the rounding of the two passes."""
        c, x, noise = self._latent_args(x, components, noise)
        with torch.cuda.device(x.device):
            handle = self.native_flow(c)
            z, eps, _, _ = handle.encode(x, noise)
            return handle.inverse(z, eps, 1.0)

    @torch.no_grad()
    def interpolate(self, x_a, x_b, weights, components, noise=None):
        """Latent interpolation between two batches of images: (len(weights), n, C, H, W), entry k the decode at temperature 1 of
        (1 - w_k) (z, eps)(x_a) + w_k (z, eps)(x_b) -- linear in the full latent; weights 0 and 1 return the two reconstructions."""
        c, x_a, noise = self._latent_args(x_a, components, noise)
        self._require_device(x_b)
        x_b = x_b.contiguous().float()
        if x_b.shape != x_a.shape:
            raise ValueError(f"x_a and x_b must have one shape, got {tuple(x_a.shape)} and {tuple(x_b.shape)}")
        with torch.cuda.device(x_a.device):
            handle = self.native_flow(c)
            za, ea, _, _ = handle.encode(x_a, noise)
            zb, eb, _, _ = handle.encode(x_b, noise)
            out = []
            for w in weights:
                w = float(w)
                # (1 - w) a + w b, not a + w (b - a): the end points are the two latents bit for bit
                out.append(handle.inverse((1.0 - w) * za + w * zb, [(1.0 - w) * p + w * q for p, q in zip(ea, eb)], 1.0))
        return torch.stack(out) if out else x_a.new_empty((0,) + tuple(x_a.shape))

    @torch.no_grad()
    def round_trip_error(self, x, components=None, noise=None):
        """The on-data invertibility check of both directions: per component max |decode(encode(x)) - u| with u = (255 x + noise) / 256,
        a device tensor (no host read).  ``components``: an int, a sequence of ints, or None = every component."""
        if components is None:
            components = range(self.num_components)
        elif isinstance(components, int):
            components = [components]
        errs = []
        for c in components:
            c, xx, nz = self._latent_args(x, int(c), noise)
            u = (255.0 * xx + (nz if nz is not None else 0.0)) / 256.0
            errs.append((self.reconstruct(xx, c, nz) - u).abs().amax() if xx.numel() else xx.new_zeros(()))
        return torch.stack(errs) if errs else x.new_zeros(0, dtype=torch.float32)

    @torch.no_grad()
    def sample(self, n=None, *, temperature=1.0, n_used=None, e=None, eps=None, uniforms=None, generator=None, return_components=False,
               y_onehot=None):
        """Images of the MIXTURE: every row through a component of its own, drawn from ``rho[0:n_used]`` per row on ``uniforms`` (n,)
        (BoostedFlow.sample; the sample(model, args) of image_experiment.py:280-293 draws one component for all rows).  ``e``: the
        standard-normal draws behind the top latents, (n,) + z_shape: rows of component c get z = mu_c + exp(lv_c) * temperature * e[rows],
        ``decode``'s formula; ``eps``: the Split2d draws, one (n, ...) tensor per level as ``decode`` takes them.  The draw and the
        partition run on the device (native.mixture_partition, one host read of the segment sizes); each component's rows are one
        ``native_flow(c).inverse`` call, gathered and written back by torch indexing.  Defaults: n = ``sample_size``, e / eps / uniforms
        from ``generator``, n_used = the trained components.  Returns x (n,C,H,W), and ``comp`` (n,) int32 with ``return_components``.
        A class-conditional model needs ``y_onehot`` (n, y_classes): row i is drawn from its component's prior of ``y_onehot[i]``."""
        n_used = self._n_used(n_used)
        temperature = 1.0 if temperature is None else float(temperature)
        dev = self.rho.device
        handles = [self.native_flow(c) for c in range(n_used)]
        y = self._y(0, y_onehot)
        for given in (e, uniforms, y) + tuple(eps or ()):
            if given is not None and n is None:
                n = given.shape[0]
        n = int(self.flows[0].sample_size) if n is None else int(n)
        if e is None:
            e = torch.randn((n,) + tuple(handles[0].z_shape), device=dev, dtype=torch.float32, generator=generator)
        if eps is None:
            eps = [torch.randn((n,) + sh, device=dev, dtype=torch.float32, generator=generator) for sh in handles[0].split_shapes()]
        if uniforms is None:
            uniforms = torch.rand(n, device=dev, dtype=torch.float32, generator=generator)
        self._require_device(e)
        if y is not None and y.shape[0] != n:
            raise ValueError(f"y_onehot must have {n} rows, got {y.shape[0]}")
        if e.shape != (n,) + tuple(handles[0].z_shape) or uniforms.shape != (n,) or any(t.shape[0] != n for t in eps):
            raise ValueError(f"e must be {(n,) + tuple(handles[0].z_shape)}, uniforms ({n},) and every eps tensor ({n}, ...)")
        e = e.contiguous().float()
        with torch.cuda.device(e.device):
            comp, order, counts, _ = native.mixture_partition(self.rho.contiguous().float(), uniforms.contiguous().float(), n_used)
            x = torch.empty((n,) + tuple(handles[0].input_size), dtype=torch.float32, device=e.device)
            begin = 0
            for c, m in enumerate(counts.cpu().tolist()):
                if m == 0:
                    continue
                rows = order[begin:begin + m]
                begin += m
                if y is not None:
                    z_c = handles[c].prior_y(y[rows].contiguous(), e[rows].contiguous(), temperature, want_prior=False)[2]
                else:
                    mu, lv = self._prior_on(handles[c], e.device)
                    z_c = mu + torch.exp(lv) * temperature * e[rows]
                x[rows] = handles[c].inverse(z_c.contiguous(), [t[rows].contiguous().float() for t in eps], temperature)
        return (x, comp) if return_components else x

    def forward(self, x=None, y_onehot=None, z=None, temperature=None, components=None, reverse=False):
        if reverse:
            return self.decode(z, y_onehot, temperature, components)
        c = self._sample_component(components) if isinstance(components, str) else int(components)
        self._require_device(x)
        if self._recording(c) or self.flows[c].y_condition:
            return self.component_forward(x, c, y_onehot=y_onehot)
        zz, ldj, _ = self.component_forward(x, c)
        handle = self.native_flow(c)
        prior = self._prior_on(handle, x.device)
        shape = (x.shape[0],) + tuple(zz.shape[1:])
        return zz, prior[0].expand(shape), prior[1].expand(shape), ldj, None      # broadcast views: same values, no copies

    @torch.no_grad()
    def _initialize_actnorms_fused(self, c, x, noise):
        """One library call for component c (gbnf_image_trainer_actnorm_init) on the component's trainer, which stays cached."""
        glow = self.flows[c]
        acts = glow._actnorms()
        skip = actnorm_skip_flags(glow)
        if all(skip):
            return
        scales = {float(m.scale) for m in acts}
        if len(scales) != 1:
            raise native.GbnfError(f"component {c}: the ActNorm2d layers have different scales {sorted(scales)}; the one-pass "
                                   "initialisation takes one (use fused=False)")
        self._row_major_1x1(glow)
        with torch.cuda.device(x.device):
            trainer, bind = self._native_trainer(c, allow_uninit=True)
            if trainer._deterministic != bool(self.image_deterministic):
                trainer.deterministic = bool(self.image_deterministic)
            for _, obj, persistent in bind:                  # the composed 1x1 matrices, as _component_forward_train brings them up to date
                if persistent is not None:
                    persistent.copy_(obj.composed_weight_tensor())
            if trainer.actnorm_count() != len(acts):
                raise native.GbnfError(f"component {c} has {len(acts)} ActNorm2d layers, the library counted {trainer.actnorm_count()}")
            trainer.actnorm_init(x, noise, scale=scales.pop(), skip=skip)
        written = [m for m, s in zip(acts, skip) if not s]
        for m in written:
            m.inited = True
        # the kernels wrote the parameters behind autograd's back (training_step does the same)
        torch.autograd.graph.increment_version([t for m in written for t in (m.bias, m.logs)])

    @torch.no_grad()
    def initialize_actnorms(self, x, components=None, noise=None, fused=False):
        """The data-dependent initialisation of every ActNorm2d of a component (the step's own and the ones behind the coupling
        nets' Conv2d layers) from the batch ``x``: what the reference's FIRST forward in training mode does, layer by layer
        (models/layers.py:473-486: bias = -mean, logs = log(scale / (sqrt(mean((x + bias)^2)) + 1e-6)) over (N, H, W), each layer
        seeing the outputs of the layers initialised before it).  The statistics come from the library
        (gbnf_image_flow_actnorm_stats, exact-f32 kernels); layers already initialised are left alone.  ``components``: an index,
        a list, or None = all.  ``noise``: the dequantisation noise (None: drawn once, as the reference's forward would).

        ``fused=True``: the whole component in ONE library call on its trainer's live tensors (gbnf_image_trainer_actnorm_init: one
        walk of the forward, statistics in f64 in a fixed order, bias / logs written on the device, no host round trip per layer);
        the trainer stays cached for the ``training_step`` that follows.  Every ActNorm2d of the component must have one ``scale``."""
        self._require_device(x)
        x = x.contiguous().float()
        noise = torch.rand_like(x) if noise is None else noise.contiguous().float()
        comps = range(self.num_components) if components is None else ([int(components)] if isinstance(components, int) else list(components))
        for c in comps:
            if fused:
                self._initialize_actnorms_fused(int(c), x, noise)
                continue
            glow = self.flows[c]
            acts = glow._actnorms()
            for idx, m in enumerate(acts):
                if m.inited:
                    continue
                # every layer not yet initialised is the identity (bias = logs = 0): mark all as usable for packing, pack on exact f32
                flags = [a.inited for a in acts]
                for a in acts:
                    a.inited = True
                try:
                    with torch.cuda.device(x.device):
                        handle = native.NativeImageFlow(image_spec_from_glow_module(glow), math="f32")
                        mean, var = handle.actnorm_stats(x, noise, idx)
                finally:
                    for a, fl in zip(acts, flags):
                        a.inited = fl
                if mean.numel() != m.num_features:
                    raise native.GbnfError(f"ActNorm2d {idx} of component {c} has {m.num_features} channels, the library counted {mean.numel()}")
                m.bias.data.copy_((-mean).view_as(m.bias))
                m.logs.data.copy_(torch.log(float(m.scale) / (torch.sqrt(var) + 1e-6)).view_as(m.logs))
                m.inited = True
        self._handles.clear()

    def component_log_prob(self, x, n_used=None, noise=None, y_onehot=None):
        """(N, C_used): ll_c = log_normal_diag(z, z_mu, z_var) + logdet (image_experiment.py:227); the SAME noise for every
        component unless the caller passes one per call.  A class-conditional model needs ``y_onehot`` (N, y_classes): ll_c is
        taken under component c's prior of each row's y."""
        n_used = self._n_used(n_used, "all")
        if noise is None:
            noise = torch.rand_like(x.float())
        y = self._y(0, y_onehot, x.shape[0])
        if y is not None:                                # (one chain after the other on the current stream)
            self._require_device(x)
            x, noise = x.contiguous().float(), noise.contiguous().float()
            with torch.cuda.device(x.device):
                return torch.stack([self.native_flow(c).forward(x, noise, want_z=False, y=y, want_logits=False)[2] for c in range(n_used)],
                                   dim=1)
        if n_used == 1:
            return self.component_forward(x, 0, noise, want_z=False)[2].unsqueeze(1)
        # the components are independent until the recursion and a component is a chain of ~50 latency-bound launches:
        # one HIP stream per component lets the chains overlap (measured: +26 % at batch 64, +13 % at 256)
        self._require_device(x)
        x = x.contiguous().float()
        noise = noise.contiguous().float()
        streams = self.__dict__.setdefault("_streams", {})
        cur = torch.cuda.current_stream(x.device)
        lls = []
        for c in range(n_used):
            st = streams.get((x.device, c))
            if st is None:
                st = streams[(x.device, c)] = torch.cuda.Stream(x.device)
            st.wait_stream(cur)
            with torch.cuda.device(x.device), torch.cuda.stream(st):
                ll = self.native_flow(c).forward(x, noise, want_z=False)[2]
            ll.record_stream(cur)
            lls.append(ll)
        for c in range(n_used):
            cur.wait_stream(streams[(x.device, c)])
        return torch.stack(lls, dim=1)

    def graphed_log_prob(self, batch, n_used=None, labels=False):
        """-> ``f(x, noise) -> G (N,)``: ``log_prob`` for batches of ``batch`` images captured ONCE in a HIP graph and
        replayed (static input / output buffers, the components' streams forked and joined inside the graph).  A component is a
        chain of ~50 short launches, so an evaluation call is host-bound as plain stream launches: the replay is 12 % faster at
        batch 256 (tools/bench_image.py, 62 -> 69.5 k images/s).  The graph holds the packed handles of the parameters it was
        captured with: ``f`` re-captures by itself when a parameter, permutation or ActNorm flag has changed since.  The
        returned tensor is the graph's output buffer -- overwritten by the next call of ``f``.  (Numerics protocol, include/gbnf.h
        gbnf_image_flow_numerics: the range marks, the repair launch and the periodic on-data check are part of every call's
        launch sequence and are counted on the device, so a replay repairs an out-of-range image exactly like a stream call; when
        an on-data check has demoted a handle, ``f`` re-captures so that the graph runs the exact-f32 kernels directly instead of
        the split-f16 pass + full repair.)  Deterministic evaluation: the graph keeps the mode its handles had when it was
        captured (``image_eval_deterministic`` at that time); changing the flag afterwards changes stream calls only -- ``f`` does NOT
        re-capture for it: build a new ``graphed_log_prob`` to have the graph in the other mode.
        ``labels=True`` (a class-conditional model): -> ``f(x, noise, y_onehot) -> G (N,)``, ``log_prob(x, noise=noise, y_onehot=y)``
        with a static (batch, y_classes) label buffer; the graph holds the components' forward_y chains one after another on one
        stream, as ``component_log_prob`` runs them for y (no parallel branches)."""
        if labels:
            self._conditioned("graphed_log_prob(labels=True)")
        elif self.flows[0].y_condition:
            raise NotImplementedError("graphed_log_prob of a class-conditional model needs the rows' labels as a graph input: pass "
                                      "labels=True for f(x, noise, y_onehot) (or use log_prob(x, y_onehot=...))")
        n_used = self._n_used(n_used, "all")
        dev = self.rho.device
        state = {}

        def handles():
            return [self.native_flow(c) for c in range(n_used)]

        def capture():
            c_, h_, w_ = self.flows[0].input_size
            xs = torch.zeros((batch, c_, h_, w_), dtype=torch.float32, device=dev)
            ns = torch.zeros_like(xs)
            ys = None
            if labels:                                           # (any valid label does for the capture: class 0 for every row)
                ys = torch.zeros((batch, int(self.flows[0].y_classes)), dtype=torch.float32, device=dev)
                ys[:, 0] = 1.0
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side), torch.no_grad():
                self.log_prob(xs, n_used, ns, ys)                # warm-up: stream creation, first-use attributes
            torch.cuda.current_stream(dev).wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g), torch.no_grad():
                out = self.log_prob(xs, n_used, ns, ys)
            # the handles the graph's kernels read are HELD here: a re-pack cannot free them (and hand their address, hence their
            # id(), to a later handle) while this graph may still be replayed
            # (... and their workspaces: a handle re-sizes its cached buffer when its deterministic mode changes)
            state.update(workspaces=[h._ws for h in handles()])
            state.update(handles=handles(), graph=g, x=xs, noise=ns, y=ys, out=out, demoted=[bool(h.numerics().demoted) for h in handles()])

        def f(x, noise, y_onehot=None):
            if tuple(x.shape) != (batch,) + tuple(self.flows[0].input_size) or tuple(noise.shape) != tuple(x.shape):
                raise native.GbnfError(f"graphed_log_prob was captured for batches of shape {(batch,) + tuple(self.flows[0].input_size)}: "
                                       f"got x {tuple(x.shape)}, noise {tuple(noise.shape)}")
            y = self._y(0, y_onehot, batch) if labels else None
            held = state.get("handles")
            now = handles()
            if (held is None or len(held) != len(now) or any(a is not b for a, b in zip(held, now))
                    or state["demoted"] != [bool(h.numerics().demoted) for h in now]):
                capture()
            state["x"].copy_(x)
            state["noise"].copy_(noise)
            if y is not None:
                state["y"].copy_(y)
            state["graph"].replay()
            return state["out"]

        return f

    def log_prob(self, x, n_used=None, noise=None, y_onehot=None):
        """(N,): log mixture density with the reference's recursion over rho (density_experiment.py:561-573); ``y_onehot`` as
        ``component_log_prob``."""
        ll = self.component_log_prob(x, n_used, noise, y_onehot)
        with torch.cuda.device(x.device):
            return native.mixture_lse(ll.t().contiguous(), self.rho)

    # ---- the score: grad_x log p(x) of a component and of the mixture (gbnf_image_mixture_score), eval or train mode
    def _score_call(self, x, comps, log_w, noise, y_onehot, want_r):
        self._require_device(x)
        x = x.detach().contiguous().float()
        if x.dim() != 4 or tuple(x.shape[1:]) != tuple(self.flows[0].input_size):
            raise ValueError(f"x must be (n, {tuple(self.flows[0].input_size)}), got {tuple(x.shape)}")
        if noise is None:
            noise = torch.rand_like(x)
        else:
            self._require_device(noise)
            if noise.shape != x.shape:
                raise ValueError(f"noise must have the shape of x, got {tuple(noise.shape)}")
            noise = noise.detach().contiguous().float()
        y = self._y(comps[0], y_onehot, x.shape[0])
        with torch.cuda.device(x.device):
            trainers = [self._step_trainer(c)[0] for c in comps]
            return native.image_mixture_score(trainers, log_w, x, noise, y=y, want_r=want_r)

    def component_score(self, x, c, noise=None, y_onehot=None):
        """-> (g_x like x, ll (N,)): the score grad_x ll_c(x) of component c and its log-density, from the exact-f32 training-path
        kernels on the live parameters with no weight gradient computed.  ``noise`` (drawn once when None) is held fixed: the
        gradient is that of the dequantised density at that noise.  Uninitialised ActNorms raise ValueError as ``training_step``."""
        c = self._check_component(c)
        g_x, ll, _ = self._score_call(x, [c], torch.zeros(1, dtype=torch.float32, device=x.device), noise, y_onehot, False)
        return g_x, ll

    def score(self, x, n_used=None, noise=None, y_onehot=None, return_log_prob=False, return_responsibilities=False):
        """grad_x log p(x) of the mixture of the first ``n_used`` components, p = sum_c w_c p_c with w_c = rho_c / sum_{j < n_used} rho_j,
        in ONE library call: sum_c r_c grad_x ll_c with the responsibilities r_c = softmax_c(log w + ll).  ``noise`` (drawn once when
        None) is shared by the components and held fixed.  -> g_x, or (g_x[, log_prob (N,)][, responsibilities (N, C_used)])."""
        n_used = self._n_used(n_used, "all")
        g_x, G, r = self._score_call(x, list(range(n_used)), self._log_w(n_used), noise, y_onehot, bool(return_responsibilities))
        return self._score_result(g_x, G, r, return_log_prob, return_responsibilities)

    def responsibilities(self, x, n_used=None, noise=None, y_onehot=None):
        """(N, C_used): p(component c | x) under the mixture ``score`` differentiates."""
        return self.score(x, n_used, noise, y_onehot, return_responsibilities=True)[1]

    # ---- label-free evaluation of a class-conditional model: the class enters a component's top prior only (models/glow.py:62-84), so
    # one pass of the flow serves every class (gbnf_image_flow_forward_classes)
    def _conditioned(self, what):
        if not self.flows[0].y_condition:
            raise ValueError(f"{what} needs a class-conditional model (y_condition): this one has no classes")

    def _class_tables(self, x, n_used, noise):
        """(C_used, N, Y) contiguous: component c's log p_c(x | y = k), one ``forward_classes`` per component on the current stream."""
        n_used = self._n_used(n_used, "all")
        self._require_device(x)
        if noise is None:
            noise = torch.rand_like(x.float())
        x, noise = x.contiguous().float(), noise.contiguous().float()
        with torch.cuda.device(x.device):
            return torch.stack([self.native_flow(c).forward_classes(x, noise)[2] for c in range(n_used)], dim=0)

    def component_class_log_prob(self, x, n_used=None, noise=None):
        """(N, C_used, Y): ``component_log_prob(x, y_onehot=e_k)[:, c]`` for every class k at once -- no labels, one flow pass per
        component instead of Y."""
        self._conditioned("component_class_log_prob")
        return self._class_tables(x, n_used, noise).permute(1, 0, 2)

    def class_log_prob(self, x, n_used=None, noise=None):
        """(N, Y): log p(x | y = k) of the boosted mixture -- ``log_prob(x, y_onehot=e_k)`` for every k -- by the recursion over rho on
        the (C, N Y) view of the components' tables (column k is bit-equal to ``native.mixture_lse`` of that column alone)."""
        self._conditioned("class_log_prob")
        t = self._class_tables(x, n_used, noise)
        with torch.cuda.device(x.device):
            return native.mixture_lse(t.view(t.shape[0], -1), self.rho).view(t.shape[1], t.shape[2])

    def _bayes(self, x, n_used, noise, class_prior, want_post, want_pred):
        table = self.class_log_prob(x, n_used, noise)
        log_prior = None
        if class_prior is not None:
            if tuple(class_prior.shape) != (table.shape[1],):
                raise ValueError(f"class_prior must be ({table.shape[1]},) probabilities, got {tuple(class_prior.shape)}")
            log_prior = torch.log(class_prior.detach().to(table.device).float()).contiguous()
        with torch.cuda.device(x.device):
            return native.class_posterior(table, log_prior, want_post=want_post, want_pred=want_pred)

    def marginal_log_prob(self, x, n_used=None, noise=None, class_prior=None):
        """(N,): log p(x) = log sum_k p(y = k) p(x | y = k), the density of unlabelled data.  ``class_prior``: (Y,) probabilities,
        None = uniform."""
        self._conditioned("marginal_log_prob")
        return self._bayes(x, n_used, noise, class_prior, False, False)[0]

    def class_posterior(self, x, n_used=None, noise=None, class_prior=None):
        """(N, Y): log p(y = k | x) of the generative classifier (Bayes' rule on ``class_log_prob``; gbnf_class_posterior)."""
        self._conditioned("class_posterior")
        return self._bayes(x, n_used, noise, class_prior, True, False)[1]

    def predict(self, x, n_used=None, noise=None, class_prior=None):
        """(N,) int64: argmax_k p(x | y = k) p(y = k), the first of the largest."""
        self._conditioned("predict")
        return self._bayes(x, n_used, noise, class_prior, False, True)[2].long()

    # ---- the mixture weights (models/boosted_flow.py:119-207)
    @torch.no_grad()
    def _rho_gradients(self, x, noise=None):
        """models/boosted_flow.py:119-139 -> (new_ll, fixed_ll, full_ll) device tensors, with the image path's own log-likelihood
        (``component_log_prob``: log_normal_diag(z, z_mu, z_var) + logdet; the reference's log_normal_standard(z, dim=-1) raises on a
        4-D z) and the reference's recursion: un-normalised rho, all three zeros where component 0 leaves them."""
        self._require_device(x)
        return self._mixture_recursion(self.component_log_prob(x, self.component + 1, noise).unbind(1))

    @torch.no_grad()
    def update_rho(self, data_loader, noise_generator=None, labels=False):
        """models/boosted_flow.py:141-207 (approximate branch) for image components.  The reference's log line references an undefined
        ``g_nll``; the update rule is reproduced, the broken log message is not.  For ``component`` >= 1 every
        iteration is ONE library call (gbnf_image_mixture_rho_step: the components' forwards, the recursion, the gradient and the
        clamped update of ``self.rho`` on the device) with step size ``rho_lr / (0.05 batch_id + 1)``; nothing is read back up to
        iteration ``min_iters`` = 10, where the reference cannot stop, and the call's 4 statistics per iteration after that.  The
        loader yields ``(x, _)`` with x in [0, 1]; the dequantisation noise is one ``torch.rand(x.shape, generator=noise_generator)``
        draw on the device per batch, the same for every component.  For ``component == 0 and all_trained`` the reference's
        gradient is identically 0 (new_ll = fixed_ll = 0): rho[0] is clamped to [0.01, 100], without a library call.
        ``labels=True`` (a class-conditional model): the loader yields ``(x, y_onehot (N, y_classes))`` and every iteration is one
        gbnf_image_mixture_rho_step_y call -- every component's ll under its prior of each row's label; everything else as above."""
        if labels:
            self._conditioned("update_rho(labels=True)")
        if self.component == 0 and not self.all_trained:
            return
        if getattr(self.args, "rho_iters", 0) == 0:
            return
        if self.flows[0].y_condition and not labels:
            raise NotImplementedError("update_rho of a class-conditional model needs the rows' labels: gbnf_image_mixture_rho_step takes "
                                      "no y (pass labels=True and a loader of (x, y_onehot))")
        self.eval()
        c = int(self.component)
        rho = self._rho_in_place("update_rho writes")
        if c == 0:
            rho[0:1].clamp_(0.01, 100.0)
            return

        def step(x, y, step_size):
            x, y, noise = self._loader_batch(x, y, labels, noise_generator)
            with torch.cuda.device(x.device):
                return native.NativeImageFlow.rho_step([self.native_flow(k) for k in range(c + 1)], x, noise, c, rho, step_size, y=y)
        self._rho_loop(data_loader, step)

    # ---- the validation pass (image_experiment.py:296-337)
    @torch.no_grad()
    def evaluate(self, data_loader, noise_generator=None, labels=False, n_used=None, y_weight=None):
        """image_experiment.py:296-337 for a boosted model, on the device: per batch the forwards of components [0, n_used), the
        recursion and the running sums in a device state, and ONE host read after the last batch.  A plain model's component chains
        overlap on their own streams as in ``component_log_prob`` and gbnf_eval_accumulate follows on the current stream; with
        ``labels`` a batch is ONE library call (gbnf_image_mixture_evaluate_y, the chains one after the other).  The reference estimates its loss from ``3 num_components`` forwards of components drawn with ``"1:c"`` per batch
        and reads it back per batch; here every component runs once and the draw is replaced by its expectation under
        w = rho[:n_used] / sum.  The loader yields ``(x, _)`` with x in [0, 1]; the dequantisation noise is one
        ``torch.rand(x.shape, generator=noise_generator)`` draw on the device per batch, the same for every component, as in
        ``update_rho``.  Default ``n_used``: all components once ``all_trained``, else ``component + 1`` -- what ``"1:c"`` draws
        from.  Puts the module in eval mode.  -> dict of floats, with D = C H W pixels:
          bpd                        the mixture's bits per dimension, -mean(G_ll) / (ln2 D)
          g_bpd                      those of component ``self.component``
          expected_component_bpd     -mean_i sum_c w_c ll_c(x_i) / (ln2 D)
          loss                       the expectation of the reference's ``avg_loss``: the mean over batches of
                                     sum_c w_c bpd_c + y_weight sum_c w_c CE_c  (the second term only with ``labels``)
          rows, batches, non_finite_rows
        ``labels=True`` (a class-conditional model): the loader yields ``(x, y_onehot (N, y_classes))``, every batch is one
        gbnf_image_mixture_evaluate_y call, and the dict also has ``loss_classes`` (the rho-weighted mean cross-entropy of
        image_experiment.py:236), ``accuracy`` (the rho-weighted share of rows whose largest logit is the label) and
        ``total_loss = bpd + y_weight loss_classes``.  ``y_weight`` defaults to ``args.y_weight``, else 0.01.  The ``multi_class``
        branch of the reference's loss is not built.  An empty loader raises ValueError."""
        if labels:
            self._conditioned("evaluate(labels=True)")
        elif self.flows[0].y_condition:
            raise NotImplementedError("evaluate of a class-conditional model needs the rows' labels: gbnf_image_mixture_evaluate takes "
                                      "no y (pass labels=True and a loader of (x, y_onehot))")
        self.eval()
        n_used, c = self._n_used(n_used), int(self.component)
        if c >= n_used:
            raise ValueError(f"component {c} is not among the first n_used = {n_used} components")
        if y_weight is None:
            y_weight = getattr(self.args, "y_weight", None)
        y_weight = 0.01 if y_weight is None else float(y_weight)
        rho = self.rho
        if rho.dtype != torch.float32 or not rho.is_contiguous():
            rho = rho.contiguous().float()
        state, pixels = None, 0
        for (x, y) in data_loader:
            x, y, noise = self._loader_batch(x, y, labels, noise_generator)
            with torch.cuda.device(x.device):
                if state is None:
                    state, pixels = native.eval_state(x.device), int(x[0].numel())
                if y is None:
                    # a plain model's chains overlap on the components' own streams (component_log_prob): a pass of 8 batches of 64
                    # through a CIFAR-shaped C = 4 model measured 12.1 ms this way and 15.7 ms with the one call's chains one after
                    # the other; the sums are the one call's: the same two launches on the same table
                    native.eval_accumulate(self.component_log_prob(x, n_used, noise).t().contiguous(), rho, c, state)
                else:
                    native.NativeImageFlow.evaluate([self.native_flow(k) for k in range(n_used)], x, noise, c, rho, state, y=y)
        s = self._eval_sums(state)          # the one host read
        rows, batches = s["rows"], s["batches"]
        per_dim = 1.0 / (math.log(2.0) * pixels)
        out = {"bpd": -s["sum_G"] / rows * per_dim, "g_bpd": -s["sum_g"] / rows * per_dim,
               "expected_component_bpd": -s["sum_E"] / rows * per_dim, "loss": -s["batch_mean_E"] / batches * per_dim,
               "rows": int(rows), "batches": int(batches), "non_finite_rows": int(s["non_finite_rows"])}
        if labels:
            out["loss"] += y_weight * s["batch_mean_ce"] / batches
            out["loss_classes"] = s["sum_ce"] / rows
            out["accuracy"] = s["sum_correct"] / rows
            out["total_loss"] = out["bpd"] + y_weight * out["loss_classes"]
        return out

    @torch.no_grad()
    def fit_weights(self, data_loader, noise_generator=None, labels=False, n_used=None, max_iters=1000, tol=1e-9, write=True):
        """All weights of the first ``n_used`` components at once, by EM with the components fixed (gbnf_weights_em): what
        ``BoostedFlow.fit_weights`` does, on the table ``component_log_prob`` writes.  No reference counterpart; it supersedes
        ``update_rho``.  One pass over the loader -- ``(x, _)`` with x in [0, 1], or ``(x, y_onehot)`` with ``labels``; the noise
        and the labels are handled as in ``evaluate`` --, every batch's ``(n_used, n)`` table copied into its columns of a device
        table of ``len(data_loader.dataset)`` columns (without a dataset the batches' tables are concatenated once), then ONE library
        call for all iterations and, with ``write``, gbnf_weights_to_rho on ``self.rho``.  ONE host read.  -> the dict of
        ``BoostedFlow.fit_weights`` (nll_* in nats per image)."""
        if labels:
            self._conditioned("fit_weights(labels=True)")
        elif self.flows[0].y_condition:
            raise NotImplementedError("fit_weights of a class-conditional model needs the rows' labels (pass labels=True and a loader "
                                      "of (x, y_onehot))")
        self.eval()
        n_used = self._n_used(n_used)

        def batch_table(x, y, table, filled):
            x, y, noise = self._loader_batch(x, y, labels, noise_generator)
            ll = self.component_log_prob(x, n_used, noise, y_onehot=y).t()
            if table is None:
                return ll
            table[:, filled:filled + x.shape[0]].copy_(ll)
        return self._fit_weights_over(data_loader, n_used, batch_table, max_iters, tol, write)

    def _loader_batch(self, x, y, labels, noise_generator):
        """A loader's ``(x, y)`` as the library calls take it: x contiguous float32 on rho's device, the labels checked with ``labels``
        (None without), and the batch's ONE draw of dequantisation noise -> (x, y, noise)."""
        dev = self.rho.device
        x = x.detach().to(dev).contiguous().float()
        self._require_device(x)
        y = self._y(0, None if y is None else y.detach().to(dev), x.shape[0]) if labels else None
        return x, y, torch.rand(x.shape, generator=noise_generator, device=x.device)

    # ---- checkpoint side-car (SURVEY.md S5 for image components)
    def _side_car_modules(self, c):
        flow = self.flows[c]
        return [m for m in flow.modules() if isinstance(m, Permute2d)], flow._actnorms()

    def permutation_state(self):
        """What the reference's checkpoints lose, in the layout of ``BoostedFlow.permutation_state``: ``component``,
        ``all_trained``, the ``Permute2d.indices`` of every step that has one and the ``inited`` flag of every ActNorm2d, keyed
        "component.position" with the position in module order.  Save next to ``state_dict()`` (``checkpoint.save`` does)."""
        st = {"component": self.component, "all_trained": self.all_trained, "indices": {}, "actnorm_inited": {}}
        for c in range(len(self.flows)):
            perms, actnorms = self._side_car_modules(c)
            for k, m in enumerate(perms):
                st["indices"][f"{c}.{k}"] = m.indices.detach().cpu().clone()
            for k, m in enumerate(actnorms):
                st["actnorm_inited"][f"{c}.{k}"] = bool(m.inited)
        return st

    def load_permutation_state(self, st):
        self.component = int(st["component"])
        self.all_trained = bool(st["all_trained"])
        touched = set()
        for name, idx in st["indices"].items():
            c, k = (int(v) for v in name.split("."))
            self._side_car_modules(c)[0][k].set_indices(idx)
            touched.add(c)
        for name, flag in st["actnorm_inited"].items():
            c, k = (int(v) for v in name.split("."))
            self._side_car_modules(c)[1][k].inited = bool(flag)
            touched.add(c)
        for c in touched:           # handles and trainers were packed with the old permutations
            self._handles.pop(c, None)
            self._trainers.pop(c, None)
