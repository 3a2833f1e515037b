"""Host-side mirror of the reference's ``BoostedFlow`` (models/boosted_flow.py) for the density path.

Same constructor (``BoostedFlow(args)`` reading the same Namespace fields), same attribute
surface (``flows``, ``rho``, ``component``, ``all_trained``, ``num_components``,
``increment_component``, ``update_rho``, ``_sample_component``), same parameter / buffer names
(``flows.<c>.flow.layers.<k>.actnorm.bias`` ..., so reference ``state_dict``s load and
optimization/optimizers.py:29-35's name parsing keeps working) and the same call:

    z, z_mu, z_var, ldj, y_logits = model(x=x, components=c)        # models/boosted_flow.py:224-228

but the arithmetic of ``self.flows[c](x)`` runs in the HIP kernels behind ``include/gbnf.h``.
The sub-modules below only HOLD parameters; they have no math of their own and there is no
CPU / eager fallback: calling the model without the built library or with CPU tensors raises.

Additions named in BASELINE.json / SURVEY.md section 8(b): ``component_forward``,
``component_log_prob``, ``log_prob`` and the permutation side-car (``permutation_state`` /
``load_permutation_state``) that fixes the reference's loss of ``PermuteNd.indices`` on checkpointing.

ActNorm's data-dependent initialisation (train mode, first batch: models/layers.py:473-486) is reproduced with
the statistics kernel ``gbnf_actnorm_init``.

Also here: the training step -- ``model.train(); model(x=x, components=c)`` is recorded by autograd
and both directions run in the library (``_FlowFunction`` / ``native.NativeTrainer``); the inverse direction / sampling
(``decode``, ``model(z=, reverse=True)``; the reference's own ``decode`` is dead code: models/boosted_flow.py:216 passes a
misspelt kwarg); image inputs dispatch to ``image_glow.BoostedImageFlow`` (``BoostedFlow.__new__``).
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import native
from . import spec as gspec
# (the three flag readers are re-exported: they are defined next to the base only to avoid an import cycle, see boosted_base.py)
from .boosted_base import BoostedMixtureBase, deterministic_from, image_deterministic_from, image_eval_deterministic_from  # noqa: F401


# ----------------------------------------------------------------------------- parameter holders

_VERSION = __import__("operator").attrgetter("_version")
_DATA_PTR = torch.Tensor.data_ptr


def _raw_stream(device):
    """The current stream's handle on ``device`` as an int (no Stream object: this runs on every module call)."""
    try:
        return torch._C._cuda_getCurrentRawStream(device.index if device.index is not None else torch.cuda.current_device())
    except AttributeError:
        return torch.cuda.current_stream(device).cuda_stream


class _ComponentTable:
    """One batch's (z, ldj) of every component in use (BoostedFlow._serve_from_table) + the ready 5-tuples the module returns.

    ``next_c``: loop mode (the default, BoostedFlow.SERVE_ALL_COMPONENTS = True) hands every entry out at most ONCE, in the
    evaluate loop's own order c = 0, 1, 2, ...: the component the table expects next; the table is dropped when the last one has
    been served.  -1 = any order, any number of times (``BoostedFlow.serving_loop()`` / SERVE_ALL_COMPONENTS = "any")."""
    __slots__ = ("xkey", "x_in", "version", "stream", "n_used", "z", "ldj", "keys", "mix", "outs", "next_c")

    def __init__(self, xkey, x_in, z, ldj, keys, mix):
        self.xkey, self.x_in, self.z, self.ldj, self.keys, self.mix = xkey, x_in, z, ldj, keys, mix
        self.version, self.n_used, self.stream = xkey[1], xkey[5], xkey[6]
        self.outs = None
        self.next_c = -1

    def serve(self, model, x, c):
        """The early look-up of BoostedFlow.forward: the same tensor object at the same version, address and shape, on the same
        stream, the same components in use, component c's parameters untouched (loop mode: and c the component that is due) -> the
        ready tuple; anything else -> None (the full path)."""
        mode = model.SERVE_ALL_COMPONENTS
        if (not 0 <= c < self.n_used or x._version != self.version or not mode
                or (self.next_c >= 0) != (mode is True) or (self.next_c >= 0 and c != self.next_c)
                or _DATA_PTR(x) != self.xkey[0] or x.shape != self.xkey[2]           # (`x.data = other`: same object and version, other storage)
                or (model.num_components if model.all_trained else model.component + 1) != self.n_used
                or _raw_stream(x.device) != self.stream or model._component_key(c) != self.keys[c]):
            return None
        out = self.outs[c]
        if self.next_c >= 0:
            self.next_c = c + 1
            if c + 1 == self.n_used:          # the loop is through: the views just handed out own the storage now
                model.__dict__.pop("_component_table", None)
        return out

class _CouplingNet(nn.Module):
    """TanhNet / ReLUNet parameter layout: ``network`` = Linear, [act, Linear] x depth, act, Linear
    (models/layers.py:208-243).  nn.Linear's default init is what the reference uses."""

    def __init__(self, in_dim, out_dim, hidden_dim, num_layers, act):
        super().__init__()
        act_cls = nn.Tanh if act == "tanh" else nn.ReLU
        layers = [nn.Linear(in_dim, hidden_dim)]
        for _ in range(num_layers):
            layers += [act_cls(), nn.Linear(hidden_dim, hidden_dim)]
        layers += [act_cls(), nn.Linear(hidden_dim, out_dim)]
        self.network = nn.Sequential(*layers)

    def forward(self, *a, **k):
        raise RuntimeError("coupling networks are evaluated by the fused HIP kernel, not module by module")


class TanhNet(_CouplingNet):
    def __init__(self, in_dim, out_dim, hidden_dim, num_layers=1):
        super().__init__(in_dim, out_dim, hidden_dim, num_layers, "tanh")


class ReLUNet(_CouplingNet):
    def __init__(self, in_dim, out_dim, hidden_dim, num_layers=1):
        super().__init__(in_dim, out_dim, hidden_dim, num_layers, "relu")


class ResidualBlock(nn.Module):
    """Parameter layout (and initialisation order) of models/layers.py:246-273: two Linear(h, h), the second one
    re-initialised uniformly in +-1e-3."""

    def __init__(self, hidden_dim):
        super().__init__()
        self.activation = nn.ReLU()
        self.linear_layers = nn.ModuleList([nn.Linear(hidden_dim, hidden_dim) for _ in range(2)])
        nn.init.uniform_(self.linear_layers[-1].weight, -1e-3, 1e-3)
        nn.init.uniform_(self.linear_layers[-1].bias, -1e-3, 1e-3)


class ResidualNet(nn.Module):
    """ResidualNet parameter layout (models/layers.py:276-301): ``initial_layer``, ``blocks`` (num_layers of them),
    ``final_layer``.  Evaluation only; RealNVP only (the reference's glow.py never imports it)."""

    def __init__(self, in_dim, out_dim, hidden_dim, num_layers=2):
        super().__init__()
        self.hidden_dim = hidden_dim
        self.initial_layer = nn.Linear(in_dim, hidden_dim)
        self.blocks = nn.ModuleList([ResidualBlock(hidden_dim) for _ in range(num_layers)])
        self.final_layer = nn.Linear(hidden_dim, out_dim)

    def forward(self, *a, **k):
        raise RuntimeError("coupling networks are evaluated by the fused HIP kernel, not module by module")


def _coupling_cls(name, realnvp=False):
    if name == "residual" and realnvp:
        return ResidualNet
    if name == "tanh":
        return TanhNet
    if name == "relu":
        return ReLUNet
    if name == "random":   # models/glow.py:295-296 draws from numpy's global RNG
        return [TanhNet, ReLUNet][np.random.randint(2)]
    if name == "residual":
        raise NotImplementedError("coupling_network='residual' with Glow: the reference's glow.py does not import "
                                  "ResidualNet (NameError there); it is available for component_type='realnvp'")
    raise NotImplementedError(
        f"coupling_network={name!r}: tanh / relu / random (and mixed / residual for RealNVP) are on the supported path")


class ActNorm1d(nn.Module):
    """Parameter holder for _ActNorm/ActNorm1d (models/layers.py:453-545): bias, logs (1,d) and
    the ``inited`` flag (a plain attribute in the reference too)."""

    def __init__(self, num_features, scale=1.0):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(1, num_features))
        self.logs = nn.Parameter(torch.zeros(1, num_features))
        self.num_features = num_features
        self.scale = scale
        self.inited = False
        self.image_input = False


class Permute1d(nn.Module):
    """PermuteNd/Permute1d (models/layers.py:633-668): ``indices`` / ``indices_inverse`` are plain
    tensors, not buffers (hence absent from state_dict -- see BoostedFlow.permutation_state)."""

    def __init__(self, num_dim, shuffle):
        super().__init__()
        self.num_dim = num_dim
        self.indices = torch.arange(num_dim - 1, -1, -1, dtype=torch.long)
        self.indices_inverse = torch.zeros(num_dim, dtype=torch.long)
        if shuffle:
            self.indices = self.indices[torch.randperm(num_dim)]
        self._rebuild_inverse()

    def __setattr__(self, name, value):
        if name == "indices":        # every (re)assignment gets a new serial number: BoostedFlow's handle keys use it
            object.__setattr__(self, "indices_serial", getattr(self, "indices_serial", 0) + 1)
        super().__setattr__(name, value)

    def _rebuild_inverse(self):
        self.indices_inverse = torch.empty(self.num_dim, dtype=torch.long)
        self.indices_inverse[self.indices] = torch.arange(self.num_dim, dtype=torch.long)

    def set_indices(self, indices):
        idx = torch.as_tensor(np.asarray(indices), dtype=torch.long).clone()
        if idx.shape != (self.num_dim,) or sorted(idx.tolist()) != list(range(self.num_dim)):
            raise ValueError("indices must be a permutation of range(num_dim)")
        self.indices = idx
        self._rebuild_inverse()


class FlowStep(nn.Module):
    """Tabular FlowStep parameter layout (models/glow.py:264-308): actnorm, shuffle|reverse, block."""

    def __init__(self, in_dim, hidden_dim, actnorm_scale, flow_permutation, flow_coupling, args):
        super().__init__()
        self.image_input = False
        self.flow_coupling = flow_coupling
        self.actnorm = ActNorm1d(in_dim, actnorm_scale)
        if flow_permutation == "shuffle":
            self.shuffle = Permute1d(in_dim, shuffle=True)
        elif flow_permutation == "invconv":
            raise NotImplementedError("invconv is image-only in the reference (models/layers.py:750 unpacks 4 dims)")
        else:
            self.reverse = Permute1d(in_dim, shuffle=False)
        net = _coupling_cls(args.coupling_network)
        d1 = in_dim // 2
        d2 = in_dim - d1
        if flow_coupling == "additive":
            self.block = net(d1, d2, hidden_dim, args.coupling_network_depth)
        elif flow_coupling == "affine":
            self.block = net(d1, d2 * 2, hidden_dim, args.coupling_network_depth)
        else:
            raise ValueError(f"flow_coupling={flow_coupling!r}")

    @property
    def permutation(self):
        return self.shuffle if hasattr(self, "shuffle") else self.reverse


class FlowNet(nn.Module):
    def __init__(self, args):
        super().__init__()
        if len(args.input_size) > 1:
            raise NotImplementedError("image inputs are built by image_glow.BoostedImageFlow (BoostedFlow(args) dispatches there)")
        self.image_input = False
        self.K = args.num_flows
        self.L = args.num_blocks
        self.output_shapes = [[-1, args.input_size[0]]]
        self.layers = nn.ModuleList([
            FlowStep(args.input_size[0], args.h_size, args.actnorm_scale, args.flow_permutation,
                     args.flow_coupling, args) for _ in range(args.num_flows)])


class Glow(nn.Module):
    """Parameter layout of the tabular Glow component (models/glow.py:12-58): flow, prior_h, bounds."""

    def __init__(self, args):
        super().__init__()
        if getattr(args, "learn_top", False) or getattr(args, "y_condition", False):
            raise NotImplementedError("learn_top / y_condition are image-path options")
        self.learn_top = False
        self.y_condition = False
        self.y_classes = args.y_classes
        self.sample_size = args.sample_size
        self.image_input = False
        self.flow = FlowNet(args)
        self.register_buffer("prior_h", torch.zeros([1, args.z_size * 2]))
        self.register_buffer("bounds", torch.tensor([0.9], dtype=torch.float32))
        self.dequant_flows = None
        self.z_size = args.z_size

    def set_actnorm_init(self):
        """Mark ActNorm layers initialised ("Use if given a loaded model", models/glow.py:181-187)."""
        for layer in self.flow.layers:
            layer.actnorm.inited = True


class BatchNorm(nn.Module):
    """RealNVP BatchNorm parameter layout (models/layers.py:320-335)."""

    def __init__(self, input_size, momentum=0.9, eps=1e-5):
        super().__init__()
        self.momentum = momentum
        self.eps = eps
        self.log_gamma = nn.Parameter(torch.zeros(input_size))
        self.beta = nn.Parameter(torch.zeros(input_size))
        self.register_buffer("running_mean", torch.zeros(input_size))
        self.register_buffer("running_var", torch.ones(input_size))
        self.register_buffer("batch_mean", torch.zeros(input_size))
        self.register_buffer("batch_var", torch.zeros(input_size))


class RealNVPFlow(nn.Module):
    """Parameter layout of RealNVPFlow (models/realnvp.py:18-78): flow_param[k] = [t_net, s_net, bn|None]."""

    def __init__(self, args, flip_init=0):
        super().__init__()
        self.num_flows = args.num_flows
        self.z_size = args.z_size
        self.flip_init = flip_init
        self.sample_size = args.sample_size
        self.register_buffer("base_dist_mean", torch.randn(self.z_size).normal_(0, 0.1))
        self.register_buffer("base_dist_var", 3.0 * torch.ones(self.z_size))
        self.flow_param = nn.ModuleList()
        for k in range(self.num_flows):
            flipped = ((k + flip_init) % 2) > 0
            if flipped:
                out_dim, in_dim = self.z_size // 2, self.z_size - self.z_size // 2
            else:
                in_dim, out_dim = self.z_size // 2, self.z_size - self.z_size // 2
            if args.coupling_network == "mixed":
                nets = [ReLUNet(in_dim, out_dim, args.h_size, args.coupling_network_depth),
                        TanhNet(in_dim, out_dim, args.h_size, args.coupling_network_depth)]
            else:
                nets = [_coupling_cls(args.coupling_network, realnvp=True)(in_dim, out_dim, args.h_size,
                                                                           args.coupling_network_depth)
                        for _ in range(2)]
            bn = BatchNorm(self.z_size) if (args.batch_norm and k < self.num_flows - 1) else None
            self.flow_param.append(nn.ModuleList(nets + [bn]))
        self.register_buffer("prior_h", torch.zeros([1, 2 * self.z_size]))


# ----------------------------------------------------------------------------- the boosted model
class _FlowFunction(torch.autograd.Function):
    """(z, ldj) = flows[c](x) recorded for autograd: forward and backward both run in libgbnf_hip.so on the live
    parameter tensors (native.NativeTrainer); activations are recomputed in the backward kernel, so only x is kept."""

    @staticmethod
    def forward(ctx, trainer, x, *params):
        z, ldj, trace = trainer.forward(x, want_trace=True)
        ctx.trainer = trainer
        ctx.trace = trace                       # every step's normalised state: spares the backward its forward sweep
        # batch-statistics BatchNorm: the step statistics live in the trainer's bound buffers (bn.batch_mean / batch_var),
        # which the NEXT recorded forward of this component overwrites -- remember which call they belong to
        trainer.forward_serial = getattr(trainer, "forward_serial", 0) + 1
        ctx.forward_serial = trainer.forward_serial
        ctx.save_for_backward(x, *params)      # params: autograd's in-place-modification check only
        return z, ldj

    @staticmethod
    def backward(ctx, g_z, g_ldj):
        x = ctx.saved_tensors[0]
        trainer = ctx.trainer
        if trainer.batch_stats and ctx.forward_serial != trainer.forward_serial:
            raise RuntimeError(
                "backward of a train-mode RealNVP component after ANOTHER recorded forward of the same component: the batch "
                "statistics of this call were overwritten (one forward -> one backward per component in batch-statistics "
                "mode; evaluate extra batches under torch.no_grad() or in eval())")
        g_z = None if g_z is None else g_z.contiguous().float()
        g_ldj = None if g_ldj is None else g_ldj.contiguous().float()
        with torch.cuda.device(x.device):
            if ctx.needs_input_grad[1] and not any(ctx.needs_input_grad[2:]) and not trainer.batch_stats:
                # no parameter asks for a gradient: the same sweeps without the weight-gradient work (gbnf_trainer_backward_x;
                # g_x has the bits of the full call)
                g_x = trainer.backward_x(x, g_z, g_ldj, trace=ctx.trace)
                return (None, g_x) + (None,) * len(ctx.needs_input_grad[2:])
            g_x, grads = trainer.backward(x, g_z, g_ldj, want_gx=ctx.needs_input_grad[1], trace=ctx.trace)
        out = [g for t, g in zip(trainer.params, grads) if t is not None]
        out = [g if need else None for g, need in zip(out, ctx.needs_input_grad[2:])]
        return (None, g_x) + tuple(out)


class BoostedFlow(BoostedMixtureBase):
    """Drop-in for models/boosted_flow.py:BoostedFlow on the density-evaluation path."""

    _CACHES = ("_tensor_cache", "_perm_cache", "_key_cache", "_prior_cache", "_component_table", "_component_meta")

    def __new__(cls, args=None, *a, **k):
        # image components (len(input_size) > 1, BASELINE.json configs[3]) live in image_glow.BoostedImageFlow
        if cls is BoostedFlow and args is not None and len(getattr(args, "input_size", [0])) > 1:
            from .image_glow import BoostedImageFlow
            return BoostedImageFlow(args)
        return super().__new__(cls)

    def __init__(self, args):
        # arithmetic of the training path (native.NativeTrainer): args.train_math, else env GBNF_TRAIN_MATH, else the fast
        # saturating "f16x3"; "bf16x6" is the range-safe trainer, "repair" f16x3 with a same-call bf16x6 re-run of a step that met the
        # range.  Checked here, before any device work.
        train_math = getattr(args, "train_math", None) or os.environ.get("GBNF_TRAIN_MATH") or "f16x3"
        if train_math not in native.NativeTrainer.TRAIN_MATH:
            raise ValueError(f"train_math must be one of {sorted(native.NativeTrainer.TRAIN_MATH)}, got {train_math!r}")
        # (`deterministic` -- gbnf_trainer_set_deterministic -- is applied to every trainer native_trainer() hands out; an unsupported
        # geometry is refused by the first training call)
        super().__init__(args)
        self.train_math = train_math
        self.amortized = not args.density_evaluation
        for c in range(self.num_components):
            if args.component_type == "realnvp":
                self.flows.append(RealNVPFlow(args, flip_init=c))
            elif args.component_type == "glow":
                self.flows.append(Glow(args))
            else:
                raise NotImplementedError("Only glow and realnvp components are currently implemented")
        self._handles_exact = {}   # c -> (version key, exact-f32 NativeFlow), inverse direction only
        self._mixture = None    # (version key, NativeMixture)
        dev = getattr(args, "device", None)
        if dev is not None:
            self.to(dev)

    # ------------------------------------------------------------------ reference API
    @property
    def base_dist(self):
        import torch.distributions as D
        return D.Normal(self.base_dist_mean, self.base_dist_var)

    def _prior_views(self, c, n):
        """Glow.prior / RealNVPFlow.prior: prior_h (zeros) repeated over the batch, returned as-is -- as broadcast VIEWS here
        (same values and shapes, no copy kernel per call), kept per (component, batch size) while prior_h is the same tensor."""
        cache = self.__dict__.setdefault("_prior_cache", {})
        ph = self.flows[c].prior_h
        hit = cache.get((c, n))
        if hit is None or hit[0] is not ph:
            h = ph.expand(n, -1)
            hit = (ph, h[:, : self.z_size], h[:, self.z_size:])
            cache[(c, n)] = hit
        return hit[1], hit[2]

    def encode(self, x, y_onehot, components):
        c = self._sample_component(components) if isinstance(components, str) else int(components)
        z, ldj = self.component_forward(x, c)
        z_mu, z_var = self._prior_views(c, x.shape[0])
        return z, z_mu, z_var, ldj, None

    @torch.no_grad()
    def decode(self, z, y_onehot, temperature, components):
        """z -> x through ONE (given or sampled) component: what models/boosted_flow.py:209-218 is meant to do (the
        reference's own call raises TypeError: :216 passes ``y_onhot=``).  ``z is None`` draws ``sample_size`` rows from
        the prior, N(0, temperature) as Glow.decode / RealNVPFlow.decode do (models/glow.py:114-116,
        models/realnvp.py:99-101: prior mean 0, "z_var" 0 -> std = exp(0) * temperature)."""
        c = self._sample_component(components) if isinstance(components, str) else int(components)
        if z is None:
            t = 1.0 if temperature is None else float(temperature)
            dev = self.rho.device
            z = torch.randn(int(self.args.sample_size), self.z_size, device=dev, dtype=torch.float32) * t
        x, _ = self.component_inverse(z, c)
        return x

    @torch.no_grad()
    def sample(self, n=None, *, temperature=None, n_used=None, z=None, uniforms=None, generator=None, return_components=False,
               return_log_prob=False):
        """Rows of the MIXTURE ``log_prob`` evaluates: every row through a component of its own, drawn from ``rho[0:n_used]`` -- what the
        TODO of models/boosted_flow.py:209-218 asks for, where ``decode`` sends all rows through ONE drawn component.  The draw is
        ``_sample_component("1:c")``'s multinomial over rho[0:n_used] / sum, per row and on the caller's ``uniforms`` (n,) in [0,1)
        (``native.resample_rows``' rule); the rows are partitioned by component on the device and each component's rows are one
        ``component_inverse``-like launch (``native.mixture_sample``: one host read of the segment sizes).  Defaults follow ``decode``:
        n = ``args.sample_size``, z = randn(n, z_size) * temperature, uniforms = rand(n) (both from ``generator``), n_used as ``log_prob``.
        Returns x (n,d), then ``comp`` (n,) int32 with ``return_components`` and ``log_prob(x, n_used)`` with ``return_log_prob``."""
        n_used = self._n_used(n_used)
        dev = self.rho.device
        if z is not None:
            n = z.shape[0]
        elif uniforms is not None and n is None:
            n = uniforms.shape[0]
        n = int(self.args.sample_size) if n is None else int(n)
        if z is None:
            t = 1.0 if temperature is None else float(temperature)
            z = torch.randn(n, self.z_size, device=dev, dtype=torch.float32, generator=generator) * t
        if uniforms is None:
            uniforms = torch.rand(n, device=dev, dtype=torch.float32, generator=generator)
        self._require_device(z)
        z = z.contiguous().float()
        uniforms = uniforms.contiguous().float()
        if z.dim() != 2 or z.shape != (n, self.z_size) or uniforms.shape != (n,):
            raise ValueError(f"z must be ({n},{self.z_size}) and uniforms ({n},), got {tuple(z.shape)} and {tuple(uniforms.shape)}")
        for c in range(n_used):
            if not all(bool(l.actnorm.inited) for l in getattr(getattr(self.flows[c], "flow", None), "layers", [])):
                raise ValueError("ActNorm not initiated: run a forward pass on data first (models/layers.py:473-475)")
        with torch.cuda.device(z.device):
            flows = [self.native_flow(c) for c in range(n_used)]
            x, _, comp = native.mixture_sample(flows, self.rho.contiguous().float(), uniforms, z, n_used=n_used, want_ldj=False)
        out = (x,)
        if return_components:
            out += (comp,)
        if return_log_prob:
            out += (self.log_prob(x, n_used),)
        return out[0] if len(out) == 1 else out

    def forward(self, x=None, y_onehot=None, z=None, temperature=None, components=None, reverse=False):
        if reverse:
            return self.decode(z, y_onehot, temperature, components)
        # the evaluate loop's calls 2 .. C of a batch (density_experiment.py:562-563): the SAME tensor object again, another
        # component -- answered from the batch's table before anything else is looked at (see _serve_from_table)
        tab = self.__dict__.get("_component_table")
        if tab is not None and x is tab.x_in and type(components) is int and not self.training:
            out = tab.serve(self, x, components)
            if out is not None:
                return out
        return self.encode(x, y_onehot, components)

    @torch.no_grad()
    def _rho_gradient_g(self, x):
        """models/boosted_flow.py:98-107 (its only callers are commented out upstream, :180): log-density of x under the NEW
        component, log N(z; 0, I) + ldj of ``forward(x, components="c")``."""
        z_g, _, _, ldj_g, _ = self.forward(x=x, components="c")
        return (torch.sum(-0.5 * math.log(2 * math.pi) - 0.5 * z_g * z_g, dim=-1) + ldj_g).detach()

    @torch.no_grad()
    def _rho_gradient_G(self, x):
        """models/boosted_flow.py:109-118: the same under ONE fixed component drawn from rho ("-c" once all are trained, else
        "1:c-1") -- the draw is the reference's torch.multinomial (_sample_component)."""
        fixed = "-c" if self.all_trained else "1:c-1"
        z_G, _, _, ldj_G, _ = self.forward(x=x, components=fixed)
        return (torch.sum(-0.5 * math.log(2 * math.pi) - 0.5 * z_G * z_G, dim=-1) + ldj_G).detach()

    @torch.no_grad()
    def _rho_gradients(self, x):
        """models/boosted_flow.py:119-139 (note: un-normalised rho in this recursion, as in the reference)."""
        self._require_device(x)
        x = x.contiguous().float()

        def columns():
            for c in range(self.component + 1):
                self._ensure_actnorm(x, c)
                with torch.cuda.device(x.device):     # ll_c = log N(z;0,I) + ldj straight from the flow kernel
                    ll = self.native_flow(c).forward(x, want_z=False, want_ldj=False, want_ll=True)[2]
                yield ll
        return self._mixture_recursion(columns())

    def update_rho(self, data_loader, fused=False):
        """models/boosted_flow.py:141-207 (approximate branch).  The reference's log line references an
        undefined ``g_nll`` and so raises NameError whenever rho_iters > 0; the update rule
        itself is reproduced, the broken log message is not.
        ``fused=True``: every iteration is one library call (gbnf_mixture_rho_step: one flow launch for all components, the
        recursion, the gradient and the clamped update of ``self.rho`` on the device); nothing is read back up to iteration
        ``min_iters``, where the reference cannot stop, and the call's 4 statistics per iteration after that."""
        if self.component == 0 and not self.all_trained:
            return
        if getattr(self.args, "rho_iters", 0) == 0:
            return
        self.eval()
        if fused and self.component > 0:
            return self._update_rho_fused(data_loader)
        with torch.no_grad():
            tolerance, min_iters = self.RHO_TOLERANCE, self.RHO_MIN_ITERS
            init_step, max_iters = self.args.rho_lr, self.args.rho_iters
            prev_rho = self.rho[self.component].item()
            batches = self._cycle(data_loader)
            for batch_id in range(max_iters):
                (x, _) = next(batches)
                x = x.detach().to(self.rho.device)
                g_ll, G_ll, _ = self._rho_gradients(x)
                gradient = torch.mean((-g_ll) - (-G_ll)).item()
                step = init_step / (0.05 * batch_id + 1)
                rho = min(max(prev_rho - step * gradient, 0.01), 100.0)
                self.rho[self.component] = rho
                dif = abs(prev_rho - rho)
                prev_rho = rho
                if batch_id > min_iters and (batch_id > max_iters or dif < tolerance):
                    break

    @torch.no_grad()
    def _update_rho_fused(self, data_loader):
        """The loop of ``update_rho`` on gbnf_mixture_rho_step, for ``self.component`` >= 1."""
        c = int(self.component)
        rho = self._rho_in_place("update_rho(fused=True) writes")

        def step(x, _, step_size):
            x = x.detach().to(rho.device).contiguous().float()
            self._require_device(x)
            for k in range(c + 1):
                self._ensure_actnorm(x, k)
            with torch.cuda.device(x.device):
                return self.native_mixture(c + 1).rho_step(x, c, rho, step_size)
        self._rho_loop(data_loader, step)

    # ------------------------------------------------------------------ native handles
    def _component_tensors(self, c):
        """(parameters, buffers, glow layers) of component c, collected once: walking the module tree costs ~0.4 ms,
        and the keys below are evaluated several times per training step.  Parameter OBJECTS are stable (optimisers
        update in place, load_state_dict copies in place); `_apply` (.to / .cuda / .float) drops the cache."""
        cache = self.__dict__.setdefault("_tensor_cache", {})
        if c not in cache:
            flow = self.flows[c]
            layers = list(flow.flow.layers) if self.component_type == "glow" else []
            cache[c] = (list(flow.parameters()), list(flow.buffers()), layers)
        return cache[c]

    def train(self, mode=True):
        """nn.Module.train, plus a look at the library's range counter where the reference's loop switches modes anyway (once per epoch:
        density_experiment.py:336 ``model.train()``, :545 ``model.eval()``).  The TRAINING kernels saturate a split-f16 operand beyond
        +-65504 instead of repairing the sample (include/gbnf.h, gbnf_training_saturation_count: their own counter -- an evaluation launch
        in between, e.g. the fixed components' boosting weights, repairs what it marks and does not count here): the step stays finite
        and its gradients are wrong for those samples.  Leaving training mode with more such waves than it began with is reported (a
        RuntimeWarning: the counter is per device, not per model).  ``BoostedFlow.check_numerics()`` is the strict form."""
        mode = bool(mode)
        out = super().train(mode)
        try:
            on_device = self.rho.is_cuda
        except AttributeError:                 # (nn.Module.__init__ -> not constructed yet)
            return out
        if on_device:
            snap = self.__dict__.get("_sat_at_train")
            if mode and snap is None:
                self.__dict__["_sat_at_train"] = self._range_counter()
            elif not mode and snap is not None:
                del self.__dict__["_sat_at_train"]
                now = self._range_counter()
                if now is not None and now > snap:
                    import warnings
                    warnings.warn(f"{now - snap} wave(s) of TRAINING kernels met a split-f16 operand beyond +-65504 while the model was in "
                                  "training mode: they saturate there -- the steps stayed finite, the gradients of those samples were wrong.  An "
                                  "exploding model (activations, gradients or weights beyond the fp16 range) or inputs far off the scale the "
                                  "flow was fitted on: normalise the inputs, lower the learning rate", RuntimeWarning, stacklevel=2)
        return out

    def _range_counter(self):
        try:
            with torch.cuda.device(self.rho.device):
                return native.training_saturation_count(reset=False)
        except Exception:                      # (no library / no device: the calls that need them raise on their own)
            return None

    def load_state_dict(self, *a, **k):
        for name in self._CACHES:      # (assign=True swaps tensor objects)
            self.__dict__.pop(name, None)
        return super().load_state_dict(*a, **k)

    def _component_key(self, c):
        """What a packed handle of component c depends on: every tensor's version counter and address, every permutation
        (its serial and its tensor's version), every ActNorm's `inited` flag.  Built on every call of the module (40 tensors:
        this is host time of the reference's evaluate loop), so attribute walks through nn.Module.__getattr__ are done once
        per tensor cache, not per call."""
        kc = self.__dict__.setdefault("_key_cache", {}).get(c)
        if kc is None:
            params, buffers, layers = self._component_tensors(c)
            perms = self.__dict__.setdefault("_perm_cache", {})
            if c not in perms:
                # (permutation, actnorm, its index tensor): `perm.indices` is a buffer -- an nn.Module.__getattr__ walk per access, 5
                # per component and call -- so the tensor object is kept.  Re-assigning `perm.indices` bumps the serial, the key changes,
                # and native_flow drops this cache before it re-packs (`_forget_component`).
                perms[c] = [(layer.permutation, layer.actnorm, layer.permutation.indices) for layer in layers]
            kc = (params + buffers, params, perms[c])
            self.__dict__["_key_cache"][c] = kc
        tensors, params, perms = kc
        # (C-level loops: 40 tensors cost ~8 us here against ~14 us as list comprehensions -- this runs on every module call)
        key = (tuple(map(_VERSION, tensors)), tuple(map(_DATA_PTR, params)))
        if perms:                         # a permutation is identified by its tensor and that tensor's version counter
            key += tuple([(p.indices_serial, t._version, bool(a.inited)) for p, a, t in perms])
        return key

    def _forget_component(self, c):
        """Drop the per-component tensor look-ups of the key (a key mismatch may mean a tensor OBJECT was replaced)."""
        for name in ("_key_cache", "_perm_cache", "_tensor_cache"):
            self.__dict__.get(name, {}).pop(c, None)

    def _needs_grad(self, x, c):
        """True when the call must be recorded by autograd: TRAIN mode, gradients enabled and the input or a parameter
        of component c asks for one (the training step of density_experiment.py:366-374).  In eval() mode the module
        is a density evaluator: calls run on the packed kernels and return tensors without autograd history (the
        reference's evaluate() detaches them anyway, density_experiment.py:558-603); ask for a recorded call in eval
        mode explicitly with ``component_forward(x, c, differentiable=True)``."""
        if not (self.training and torch.is_grad_enabled()):
            return False
        return bool(x.requires_grad) or any(p.requires_grad for p in self._component_tensors(c)[0])

    def native_trainer(self, c):
        """The training-path handle of component c: bound to the parameter tensors' device addresses, re-created only
        when a tensor is re-allocated or a permutation changes (in-place optimiser updates need nothing)."""
        flow = self.flows[c]
        params, buffers, layers = self._component_tensors(c)
        key = [t.data_ptr() for t in params] + [t.data_ptr() for t in buffers]
        key += [(layer.permutation.indices_serial, int(layer.permutation.indices._version)) for layer in layers]
        key = tuple(key)
        cached = self._trainers.get(c)
        if cached is None or cached[0] != key:
            # (a geometry without the kernels of self.train_math raises GbnfError here: the module never downgrades the mode)
            self._trainers[c] = (key, native.NativeTrainer(gspec.device_spec_from_component(flow), math=self.train_math))
        trainer = self._trainers[c][1]
        if trainer._deterministic != bool(self.deterministic):         # (also a cached trainer after the module's flag changed)
            trainer.deterministic = bool(self.deterministic)
        return trainer

    def _ensure_actnorm(self, x, c):
        """_ActNorm.forward initialises itself from the first batch it sees in TRAIN mode and raises in eval mode
        (models/layers.py:473-486, 524-525).  Here: layer k of component c is initialised from the output of the
        first k (already initialised) steps, computed by the HIP path, with the statistics kernel
        gbnf_actnorm_init."""
        if self.component_type != "glow":
            return
        cached = self.__dict__.get("_perm_cache", {}).get(c)          # (built by _component_key: no module-tree walk per call)
        if cached is not None and all(a.inited for _, a, _t in cached):
            return
        layers = self.flows[c].flow.layers
        if all(bool(l.actnorm.inited) for l in layers):
            return
        if not self.training:
            raise ValueError("In Eval mode, but ActNorm not initiated")
        with torch.no_grad(), torch.cuda.device(x.device):
            for k, layer in enumerate(layers):
                if layer.actnorm.inited:
                    continue
                if k == 0:
                    zk = x
                else:
                    head = gspec.spec_from_glow_module(self.flows[c], upto=k)
                    zk, _, _ = native.NativeFlow(head).forward(x, want_ldj=False)
                bias, logs = native.actnorm_init(zk.contiguous(), layer.actnorm.scale)
                layer.actnorm.bias.copy_(bias.view(1, -1))
                layer.actnorm.logs.copy_(logs.view(1, -1))
                layer.actnorm.inited = True

    def native_flow(self, c):
        key = self._component_key(c)
        cached = self._handles.get(c)
        if cached is None or cached[0] != key:
            self._forget_component(c)
            key = self._component_key(c)
            math = self.__dict__.setdefault("_math_override", {}).get(c, "default")
            handle = native.NativeFlow(gspec.spec_from_component(self.flows[c]), math=math,
                                       per_step_activation=self._per_step_activation())
            self._handles[c] = (key, handle)
            self._mixture = None
            self.__dict__.setdefault("_calibrated", set()).discard(c)
        return self._handles[c][1]

    # How the evaluation kernels keep the 1e-5 bar:
    #   range      an operand beyond the fp16 range is repaired on the device by the bf16x6 pass behind every f16x3 launch;
    #   precision  at creation the library probes every component (N(0,1) / N(0,4) rows) on the f16x3 and the bf16x6
    #              packing and keeps f16x3 only when they agree to 2.5e-6 (GBNF_MATH_DEFAULT);
    #   data       the LIBRARY re-checks the choice on the caller's data, on the device and without a synchronisation: the
    #              first launch of every handle and every 256th evaluate <= 256 rows on both packings; a failed check
    #              re-evaluates that launch on bf16x6 and moves the handle there for good (include/gbnf.h,
    #              gbnf_numerics_status; `numerics_status()` below).  Round 2 did this check here, in Python, for module
    #              callers only; `verify_numerics` remains as the explicit, synchronous form.
    NUMERICS_TOL = 2.5e-6

    def numerics_status(self, n_used=None, direction="forward"):
        """State of the library's numerics guard for the mixture of the first n_used components (no synchronisation):
        dict(math_mode, demoted, checks, worst_rel_err, tolerance).  ``direction="inverse"``: the same keys for the z -> x
        direction, which runs per component (``component_inverse``): the worst over the first n_used components' own guards
        (gbnf_flow_numerics_inverse) -- demoted if any is, checks summed, the largest worst_rel_err (max(e_l, e_x / 2), against the
        log|det| tolerance)."""
        if native.check_direction(direction) == "inverse":
            sts = [self.native_flow(c).numerics("inverse") for c in range(self._n_used(n_used))]
            return {"math_mode": native.MATH_NAME[max(int(st.math_mode) for st in sts)], "demoted": any(bool(st.demoted) for st in sts),
                    "checks": sum(int(st.checks) for st in sts), "worst_rel_err": max(float(st.worst_rel_err) for st in sts),
                    "tolerance": float(sts[0].tolerance)}
        st = self.native_mixture(self._n_used(n_used)).numerics()
        return {"math_mode": native.MATH_NAME[int(st.math_mode)], "demoted": bool(st.demoted), "checks": int(st.checks),
                "worst_rel_err": float(st.worst_rel_err), "tolerance": float(st.tolerance)}

    @torch.no_grad()
    def verify_numerics(self, x, components=None, rows=256):
        """Largest relative log-likelihood difference between the packing each component runs on and its bf16x6 packing,
        on (the first `rows` rows of) x; components beyond NUMERICS_TOL are re-packed as bf16x6 from now on."""
        self._require_device(x)
        xs = x[:rows].contiguous().float()
        comps = range(self.num_components) if components is None else components
        worst = 0.0
        done = self.__dict__.setdefault("_calibrated", set())
        for c in comps:
            flow = self.native_flow(c)
            done.add(c)
            if flow.info().math_mode != native.MATH["f16x3"] or xs.shape[0] == 0:
                continue
            with torch.cuda.device(xs.device):
                safe = native.NativeFlow(gspec.spec_from_component(self.flows[c]), math="bf16x6",
                                         per_step_activation=self._per_step_activation())
                a = flow.forward(xs, want_z=False, want_ldj=False, want_ll=True)[2]
                b = safe.forward(xs, want_z=False, want_ldj=False, want_ll=True)[2]
            fin = torch.isfinite(a) & torch.isfinite(b)
            err = float(((a - b).abs() / b.abs().clamp_min(1.0))[fin].max()) if bool(fin.any()) else 0.0
            if bool((torch.isfinite(a) != torch.isfinite(b)).any()):
                err = float("inf")
            worst = max(worst, err)
            if err > self.NUMERICS_TOL:
                self.__dict__.setdefault("_math_override", {})[c] = "bf16x6"
                self._handles[c] = (self._handles[c][0], safe)
                self._mixture = None
        return worst

    def _guard(self, x, comps):
        """(The data check lives in the library since round 3: every handle checks its own first launch on the device.)"""
        return

    def _per_step_activation(self):
        """`--coupling_network random`: components (or the steps of one) differ in activation, so every handle is packed
        for the kernel variants that read it per step and all of them still share one mixture launch."""
        if getattr(self, "_per_step_act", None) is None:
            pats = {gspec.activation_pattern_of_component(self.flows[c]) for c in range(self.num_components)}
            self._per_step_act = len(pats) > 1 or any(len(set(p)) > 1 for p in pats)
        return self._per_step_act

    def native_flow_exact(self, c):
        """The exact-f32 handle of component c (ResidualNets; the other architectures run either direction on their
        evaluation handle since round 3)."""
        key = self._component_key(c)
        cached = self._handles_exact.get(c)
        if cached is None or cached[0] != key:
            self._handles_exact[c] = (key, native.NativeFlow(gspec.spec_from_component(self.flows[c]), math="f32"))
        return self._handles_exact[c][1]

    def native_mixture(self, n_used=None):
        """The mixture handle over components [0, n_used) (default: all).  Only those components' handles are looked at:
        while component c is being trained its parameters change every step, and re-packing it for a mixture that
        only needs the c FIXED components (boosting_weights) would cost a host pack + upload per step."""
        n_used = self.num_components if n_used is None else int(n_used)
        flows = [self.native_flow(c) for c in range(n_used)]
        key = tuple(id(f) for f in flows)
        cached = None if self._mixture is None else self._mixture.get(n_used)
        if cached is None or cached[0] != key:
            try:
                mix = native.NativeMixture(flows)
            except native.GbnfError:
                if self._per_step_activation():
                    raise
                # components ended up on different kernel variants: put all of them on the per-step-activation supersets
                self._per_step_act = True
                self._handles = {}
                flows = [self.native_flow(c) for c in range(n_used)]
                key = tuple(id(f) for f in flows)
                mix = native.NativeMixture(flows)
            if self._mixture is None:
                self._mixture = {}
            self._mixture[n_used] = (key, mix)
            cached = self._mixture[n_used]
        return cached[1]

    # ------------------------------------------------------------------ convenience API (BASELINE.json)
    def component_forward(self, x, c, differentiable=None):
        """x (N,d) -> z (N,d), ldj (N,) of component c  ==  self.flows[c](x)[0], [3] of the reference.
        ``differentiable``: None = recorded by autograd in train mode only (see ``_needs_grad``); True / False force it."""
        self._require_device(x)
        x_in = x
        x = x.contiguous().float()
        self._ensure_actnorm(x, int(c))
        with torch.cuda.device(x.device):
            if self._needs_grad(x, int(c)) if differentiable is None else bool(differentiable):
                trainer = self.native_trainer(int(c))
                # train(): BatchNorm normalises with the batch statistics and updates its running ones (models/layers.py:338-346)
                batch_stats = bool(self.training and trainer.has_batch_stats)
                trainer.set_batch_stats(batch_stats)
                params = [t for t in trainer.params if t is not None]
                out = _FlowFunction.apply(trainer, x, *params)
                if batch_stats:
                    with torch.no_grad():
                        for mods in self.flows[int(c)].flow_param:
                            bn = mods[2] if len(mods) > 2 else None
                            if bn is not None:
                                bn.running_mean.mul_(bn.momentum).add_(bn.batch_mean * (1 - bn.momentum))
                                bn.running_var.mul_(bn.momentum).add_(bn.batch_var * (1 - bn.momentum))
                return out
            self._guard(x, [int(c)])
            served = None if differentiable else self._serve_from_table(x, int(c), x_in)
            if served is not None:
                return served
            z, ldj, _ = self.native_flow(int(c)).forward(x)
        return z, ldj

    def training_step(self, x, *, lr, weight_decay=0.0, max_grad_norm=0.0, optimizer="adamw", betas=(0.9, 0.999), eps=1e-8,
                      resample=None, beta=1.0, uniforms=None):
        """The body of one iteration of the reference's training loop (density_experiment.py:340-384) for ``self.component``, in one
        library call (gbnf_trainer_nll_step): compute_kl_pq_loss (:606-674) -- for a boosted component beyond the first on the batch
        resampled with ``boosting_weights`` and the CALLER's RNG (``torch.multinomial``) --, ``nll.backward()``, ``clip_grad_norm_``
        (``max_grad_norm`` > 0) and the step of ``optim.AdamW`` / ``optim.SGD`` ("adamw" | "sgd") on the component's parameters, in
        place.  ``lr`` is per call (schedulers stay with the caller; a component that is not being trained gets 0).  ``resample``
        defaults to ``self.component > 0 or self.all_trained``.  ActNorm's data-dependent initialisation and the BatchNorm mode follow
        ``component_forward``; in train() mode the running statistics are updated on the device.  Returns 0-dim DEVICE tensors (nothing
        is read back): ``nll``, ``grad_norm``, ``clip_coef`` and, when resampled, ``G_nll``.  The optimiser state is kept per component
        (``self.opt_state(c)``: a ``native.OptState``).  No ``p.grad`` is written.
        ``uniforms``: the draws of the resample.  None (the default) keeps ``torch.multinomial`` and three library calls.  A (n,) float32
        device tensor of values in [0,1), or True for ``torch.rand(n, device=...)``, takes the boosted step in ONE library call
        (gbnf_boosted_nll_step: mixture log-density, weights, inverse-CDF resample on these uniforms, the step); the result gains ``ess``,
        the effective sample size of the weights, and all five entries are views of one stats tensor.  The first component has nothing
        to resample from and ignores it."""
        self._require_device(x)
        c = int(self.component)
        x = x.contiguous().float()
        self._ensure_actnorm(x, c)
        if resample is None:
            resample = bool(self.component > 0 or self.all_trained)
        out, rows = {}, None
        if resample and uniforms is not None and c > 0:
            return self._boosted_training_step(x, c, uniforms, beta, optimizer,
                                               dict(lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm, betas=betas, eps=eps))
        if resample:
            with torch.no_grad():
                w, G = self.boosting_weights(x, beta)
                rows = torch.multinomial(w, x.shape[0], replacement=True)
                out["G_nll"] = -G.mean()
        with torch.cuda.device(x.device):
            trainer = self.native_trainer(c)
            batch_stats = bool(self.training and trainer.has_batch_stats)
            trainer.set_batch_stats(batch_stats)
            trainer.forward_serial = getattr(trainer, "forward_serial", 0) + 1     # (the bound batch statistics are overwritten)
            state = self.opt_state(c, optimizer)
            momentum = -1.0
            if batch_stats:
                momentum = next(float(m[2].momentum) for m in self.flows[c].flow_param if len(m) > 2 and m[2] is not None)
            stats, _ = trainer.nll_step(x, state, rows=rows, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                                        betas=betas, eps=eps, bn_momentum=momentum)
        # the kernels wrote the parameters (and running statistics) behind autograd's back: move their version counters, on the host
        # and without a launch, so that every packed evaluation copy keyed on them (_component_key) is rebuilt
        params, buffers, _ = self._component_tensors(c)
        torch.autograd.graph.increment_version(params + buffers if batch_stats else params)
        out.update(nll=stats[0], grad_norm=stats[1], clip_coef=stats[2])
        return out

    def _boosted_training_step(self, x, c, uniforms, beta, optimizer, hyper):
        """``training_step`` of component c > 0 on given uniforms: one gbnf_boosted_nll_step."""
        n = x.shape[0]
        u = torch.rand(n, device=x.device) if uniforms is True else uniforms
        if not isinstance(u, torch.Tensor) or u.shape != (n,) or u.dtype != torch.float32 or u.device != x.device:
            raise ValueError(f"uniforms must be True or a ({n},) float32 tensor on {x.device}")
        for k in range(c):
            self._ensure_actnorm(x, k)
        self._guard(x, range(c))
        with torch.cuda.device(x.device):
            mixture = self.native_mixture(c)
            trainer = self.native_trainer(c)
            batch_stats = bool(self.training and trainer.has_batch_stats)
            trainer.set_batch_stats(batch_stats)
            trainer.forward_serial = getattr(trainer, "forward_serial", 0) + 1     # (the bound batch statistics are overwritten)
            state = self.opt_state(c, optimizer)
            momentum = -1.0
            if batch_stats:
                momentum = next(float(m[2].momentum) for m in self.flows[c].flow_param if len(m) > 2 and m[2] is not None)
            stats, _, _ = trainer.boosted_nll_step(mixture, c, self.rho.contiguous().float(), x, u.contiguous(), state, beta=beta,
                                                   bn_momentum=momentum, **hyper)
        params, buffers, _ = self._component_tensors(c)
        torch.autograd.graph.increment_version(params + buffers if batch_stats else params)
        return {"G_nll": stats[4], "ess": stats[5], "nll": stats[0], "grad_norm": stats[1], "clip_coef": stats[2]}

    def mixture_training_step(self, x, *, lr, weight_decay=0.0, max_grad_norm=0.0, optimizer="adamw", betas=(0.9, 0.999), eps=1e-8,
                              n_used=None):
        """One JOINT step of components 0 .. ``n_used`` - 1 (default as ``log_prob``) on the objective the model is judged by, the
        mixture likelihood  -mean_i log sum_c w_c p_c(x_i), in one library call (gbnf_mixture_nll_step): every component's forward,
        the responsibilities r = softmax_c(log w + ll), every component's backward on the seeds (r_c / n) z_c, -r_c / n, ONE clip
        coefficient over all components' gradients (``clip_grad_norm_(model.parameters())``) and every component's ``optim.AdamW`` /
        ``optim.SGD`` update, in place.  No reference counterpart (the reference trains one component at a time); what it replaces
        is the eager composition of C recorded forwards, a logsumexp, backward, clip and C optimiser steps.  The weights are
        w_c = rho_c / sum_{j < n_used} rho_j (``score``'s closed form), held fixed during the step.  ``lr``: a float, or ``n_used``
        floats (0: that component's parameters stay bit for bit while its moments move).  The optimiser states are
        ``self.opt_state(c, optimizer)``, so a boosted model continues on the moments ``training_step`` left.  Runs on the RUNNING
        statistics in either module mode (the trainers' batch-statistics mode is switched off for the call and put back; a recorded
        train-mode forward still awaiting its backward raises RuntimeError on that backward, as with ``score``); uninitialised
        ActNorms raise ValueError.  Returns device tensors, nothing is read back: ``nll``, ``grad_norm`` (over all components),
        ``clip_coef`` (0-dim), ``mean_responsibilities`` (n_used,) and ``component_grad_norms`` (n_used,).
        ``mean_responsibilities`` is the EM update of the weights on this batch (``fit_weights`` does the same over a whole table):
        a caller who wants a stochastic weight update between ``fit_weights`` calls has it here.  No ``p.grad`` is written."""
        n_used = self._n_used(n_used)
        comps = list(range(n_used))
        x = self._score_input(x, comps)
        lrs = [float(lr)] * n_used if isinstance(lr, (int, float)) else [float(v) for v in lr]
        if len(lrs) != n_used:
            raise ValueError(f"lr must be a float or {n_used} floats (one per component in use), got {len(lrs)}")
        with torch.cuda.device(x.device):
            trainers = [self.native_trainer(c) for c in comps]
            states = [self.opt_state(c, optimizer) for c in comps]
            modes = [t.batch_stats for t in trainers]
            try:
                for t in trainers:
                    t.set_batch_stats(False)
                    if t.has_batch_stats:
                        t.forward_serial = getattr(t, "forward_serial", 0) + 1
                stats, _, _, _ = native.mixture_nll_step(trainers, states, self._log_w(n_used), x, lr=lrs, weight_decay=weight_decay,
                                                         max_grad_norm=max_grad_norm, betas=betas, eps=eps)
            finally:
                for t, on in zip(trainers, modes):
                    t.set_batch_stats(on)
        # the kernels wrote the parameters behind autograd's back: move their version counters so that the packed evaluation copies
        # keyed on them (_component_key) are rebuilt
        params = [p for c in comps for p in self._component_tensors(c)[0]]
        torch.autograd.graph.increment_version(params)
        return {"nll": stats[0], "grad_norm": stats[1], "clip_coef": stats[2], "mean_responsibilities": stats[4:4 + n_used],
                "component_grad_norms": stats[4 + n_used:4 + 2 * n_used]}

    def opt_state(self, c, optimizer="adamw"):
        """The ``native.OptState`` ``training_step`` keeps for component c (created on first use; another ``optimizer`` kind or a
        re-shaped component starts a new one)."""
        trainer = self.native_trainer(int(c))
        states = self.__dict__.setdefault("_opt_states", {})
        st = states.get(int(c))
        if st is None or st.kind != optimizer or st.grad_floats != trainer.grad_floats or st.exp_avg_device != trainer.device:
            st = states[int(c)] = native.OptState(trainer, optimizer)
        return st

    # The reference's evaluate loop asks for the components of ONE batch one call at a time
    # (density_experiment.py:561-573: ``for c in range(model.component + 1): model(x=x, components=c)``).  All of them read
    # the same x, so in eval() mode the first call of a batch launches EVERY component in use
    # (gbnf_mixture_component_forward: one launch, one (C, N, d) table) and the following calls are answered from that
    # table with no launch at all.  The table is keyed on everything a result depends on: x's storage address, shape,
    # strides and version counter (an in-place write to x bumps it), the packed handles of the components (rebuilt whenever
    # a parameter's version counter moves: an optimiser step, load_state_dict, a new permutation), and the stream.
    # SERVE_ALL_COMPONENTS (VERDICT r5 item 9 / ADVICE r4: the cache is scoped):
    #   True (default) -- LOOP mode.  A table is started by a call for component 0 and serves the evaluate loop's own sequence
    #       c = 1, 2, ..., n_used - 1 on the same tensor: every entry is handed out at most ONCE and the table is dropped with the
    #       last one.  So the (z, ldj) views a caller gets are never handed to anybody else (editing them in place is as safe as
    #       editing the reference's fresh tensors), nothing of a batch outlives its loop (a write that bypasses the version counter
    #       BETWEEN two loops -- ``x.data.copy_``, a graph replay into a static input buffer, a raw-pointer write -- is seen,
    #       because the next loop starts a new table), a repeated or out-of-order call takes the plain one-component path, and
    #       the (C, N, d) table is freed as soon as the loop is through.  What it still cannot see: such a bypassing write in the
    #       MIDDLE of one loop over one batch.
    #   "any" / ``with model.serving_loop():`` -- any component, any order, any number of times from the batch's table until
    #       another batch comes in (rounds 4-5's behaviour): for callers that own x and do not write to it behind the version
    #       counter; the served tensors are shared views (clone before editing); ``drop_component_table()`` frees the table.
    #   False -- never: every call launches its own component.
    SERVE_ALL_COMPONENTS = True

    def serving_loop(self):
        """Context manager: inside it every eval()-mode ``model(x=x, components=c)`` call on one batch tensor is answered from ONE
        launch's table in any order and any number of times (SERVE_ALL_COMPONENTS = "any"); the table is dropped on exit."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            before = self.__dict__.get("SERVE_ALL_COMPONENTS", None)
            self.SERVE_ALL_COMPONENTS = "any"
            try:
                yield self
            finally:
                self.drop_component_table()
                if before is None:
                    self.__dict__.pop("SERVE_ALL_COMPONENTS", None)
                else:
                    self.SERVE_ALL_COMPONENTS = before
        return scope()

    def _serve_from_table(self, x, c, x_in=None):
        """(z, ldj) of component c from the table of the batch, or None when the call is not an evaluation-loop call.
        ``x_in`` is the tensor the caller handed over (the key), ``x`` its contiguous float32 form (what is launched)."""
        # eval() mode only: there the module returns tensors without autograd history whatever the grad mode is (_needs_grad;
        # the reference's evaluate() does not enter no_grad either, it detaches: density_experiment.py:545-577)
        if not self.SERVE_ALL_COMPONENTS or self.training:
            return None
        n_used = self.num_components if self.all_trained else self.component + 1
        if n_used < 2 or c >= n_used or x.shape[0] == 0:
            return None
        x_in = x if x_in is None else x_in
        mode = self.SERVE_ALL_COMPONENTS
        loop = mode is True           # loop mode: every entry once, in the order c = 0, 1, ...; a table is only ever started by c = 0
        try:
            xkey = (x_in.data_ptr(), x_in._version, x_in.shape, tuple(x_in.stride()), x_in.dtype, n_used,
                    _raw_stream(x.device))
        except RuntimeError:          # inference tensors keep no version counter: nothing to key on
            return None
        tab = self.__dict__.get("_component_table")
        if loop and tab is not None and (tab.next_c < 0 or tab.xkey != xkey or c != tab.next_c):
            # not the loop's next call (another batch, a repeated or an out-of-order component, a table of the other mode): the
            # table has served its loop -- what is left of it is never handed out
            self.__dict__.pop("_component_table", None)
            tab = None
        if loop and tab is None and c != 0:
            return None                   # a lone call for some component: the plain path launches that component alone
        if not loop and tab is not None and tab.next_c >= 0:
            tab = None
        # entry c depends on x and on component c's parameters only: one component key per call, as the plain path costs
        if tab is None or tab.xkey != xkey or tab.keys[c] != self._component_key(c):
            # A new batch.  ONE pass over the components' keys (round 5: this call was 115 us of host time -- the condition above,
            # native_mixture's walk over the handles and the ActNorm check each went through the keys / the layers again): if they
            # are the keys the previous table was built on, its mixture and its `inited` check still stand (`inited` is in the key)
            keys = [self._component_key(k) for k in range(n_used)]
            meta = self.__dict__.get("_component_meta")      # (n_used, keys, mixture) of the last table: outlives the table itself
            if meta is not None and meta[0] == n_used and meta[1] == keys and self._mixture is not None \
                    and self._mixture.get(n_used, (None, None))[1] is meta[2]:
                mix = meta[2]
            else:
                if self.component_type == "glow" and not all(
                        bool(l.actnorm.inited) for k in range(n_used) for l in self.flows[k].flow.layers):
                    return None           # the reference raises at the call of THAT component: leave it to the plain path
                mix = self.native_mixture(n_used)              # re-packs whatever changed
                keys = [self._handles[k][0] for k in range(n_used)]     # (the keys native_mixture has just validated the handles against)
            z, ldj, _ = mix.component_forward(x, 0, n_used)
            # (x_in is held: its storage cannot be freed and handed to another tensor with the same address and version)
            tab = _ComponentTable(xkey, x_in, z, ldj, keys, mix)
            zs, ls = z.unbind(0), ldj.unbind(0)
            n = x.shape[0]
            tab.outs = [(zs[k], *self._prior_views(k, n), ls[k], None) for k in range(n_used)]
            tab.next_c = 0 if loop else -1
            self.__dict__["_component_table"] = tab
            self.__dict__["_component_meta"] = (n_used, keys, mix)
        if loop:
            tab.next_c = c + 1
            if c + 1 == n_used:
                self.__dict__.pop("_component_table", None)
        return tab.z[c], tab.ldj[c]

    def drop_component_table(self):
        """Forget the table of the last batch (frees its (C, N, d) device memory)."""
        self.__dict__.pop("_component_table", None)

    def invalidate_packed(self):
        """Forget every packed copy of the parameters (evaluation handles, mixtures, the batch table): the next call re-packs from
        the live tensors.  The packed copies are keyed on the tensors' version counters, addresses and permutation serials, which
        every ordinary update moves (optimiser steps, ``load_state_dict``, ``p.add_()`` / ``p.copy_()`` under ``no_grad``, ``.to()``);
        what they CANNOT see is an in-place write through ``.data`` (``p.data.clamp_()``, ``p.data.copy_(w)``: PyTorch bumps no
        counter for it) or through a raw pointer -- call this after such a write.  (The training handles read the live tensors
        on every call and need nothing.)  ``training_step`` updates the parameters through raw pointers too; it does not call this
        but moves the version counters of the component it updated itself (``torch.autograd.graph.increment_version``: host only),
        so only that component's packed copies are rebuilt."""
        self._handles = {}
        self._handles_exact = {}
        self._mixture = None
        for name in ("_component_table", "_component_meta", "_key_cache", "_prior_cache"):
            self.__dict__.pop(name, None)

    def component_inverse(self, z, c):
        """z (N,d) -> x (N,d), log|det dx/dz| (N,) of component c: inverse of ``component_forward``."""
        self._require_device(z)
        z = z.contiguous().float()
        if not all(bool(l.actnorm.inited) for l in getattr(getattr(self.flows[int(c)], "flow", None), "layers", [])):
            raise ValueError("ActNorm not initiated: run a forward pass on data first (models/layers.py:473-475)")
        with torch.cuda.device(z.device):
            # the component's evaluation handle runs backwards too (split kernels: 3 x the exact-f32 kernel's rate)
            return self.native_flow(int(c)).inverse(z)

    def component_log_prob(self, x, n_used=None):
        """(N, C_used): ll_c(x) = log N(z_c;0,I) + ldj_c for c < n_used, all in ONE launch
        (density_experiment.py:562-565)."""
        self._require_device(x)
        n_used = self._n_used(n_used)
        x = x.contiguous().float()
        for c in range(n_used):
            self._ensure_actnorm(x, c)
        self._guard(x, range(n_used))
        with torch.cuda.device(x.device):
            ll = self.native_mixture(n_used).component_log_prob(x, 0, n_used)
        return ll.t()

    def log_prob(self, x, n_used=None):
        """(N,): mixture log-density over the first n_used components with the recursive
        prefix-normalised weights of density_experiment.py:561-573.  Default n_used: ``self.component + 1`` as the
        reference's ``evaluate`` (density_experiment.py:562), and ALL components once ``all_trained`` -- a deliberate
        divergence: the reference keeps ``range(self.component + 1)`` there too, which after the last boosting pass
        (component reset to 0) evaluates only the first component; pass ``n_used`` to reproduce that."""
        self._require_device(x)
        n_used = self._n_used(n_used)
        x = x.contiguous().float()
        for c in range(n_used):
            self._ensure_actnorm(x, c)
        self._guard(x, range(n_used))
        with torch.cuda.device(x.device):
            G, _ = self.native_mixture(n_used).log_prob(x, self.rho.contiguous().float(), n_used=n_used)
        return G

    @torch.no_grad()
    def evaluate(self, data_loader, n_used=None):
        """density_experiment.py:544-603, the boosted branch, on the device: per batch of a loader of ``(x, _)`` ONE library call
        (gbnf_mixture_evaluate: one flow launch for components [0, n_used), the recursion and the running sums in a device state),
        and ONE host read after the last batch -- where the reference runs ``component + 1`` module forwards for G and a further one
        for g per batch, a ``torch.cat`` over the whole set and ``.mean().item()``.  Puts the module in eval mode.  -> dict of floats:
          nll, g_nll, ratio          the reference's three (:582-591; ratio = mean(g_nll - G_nll); with ``component == 0 and not
                                     all_trained``: g_nll = nll, ratio = 0.0); g is ``self.component``
          expected_component_nll     -mean_i sum_c w_c ll_c(x_i), w = rho[:n_used] / sum: what drawing components "1:c" estimates
          nll_batch_mean             the mean over batches of the batch means of G_nll (the form of the non-boosted branch, :594)
          rows, batches, non_finite_rows
        Default ``n_used`` as ``log_prob`` (all components once ``all_trained``; pass ``component + 1`` for the reference's range).
        An empty loader raises ValueError."""
        self.eval()
        n_used = self._n_used(n_used)
        c = int(self.component)
        if c >= n_used:
            raise ValueError(f"component {c} is not among the first n_used = {n_used} components")
        dev = self.rho.device
        rho = self.rho.contiguous().float()
        state = None
        for (x, _) in data_loader:
            x = x.detach().to(dev)
            self._require_device(x)
            x = x.contiguous().float()
            for k in range(n_used):
                self._ensure_actnorm(x, k)
            self._guard(x, range(n_used))
            with torch.cuda.device(x.device):
                if state is None:
                    state = native.eval_state(x.device)
                self.native_mixture(n_used).evaluate(x, c, rho, state, n_used=n_used)
        s = self._eval_sums(state)          # the one host read
        rows, batches = s["rows"], s["batches"]
        out = {"nll": -s["sum_G"] / rows, "g_nll": -s["sum_g"] / rows, "ratio": s["sum_G_minus_g"] / rows,
               "expected_component_nll": -s["sum_E"] / rows, "nll_batch_mean": -s["batch_mean_G"] / batches,
               "rows": int(rows), "batches": int(batches), "non_finite_rows": int(s["non_finite_rows"])}
        if c == 0 and not self.all_trained:
            out["g_nll"], out["ratio"] = out["nll"], 0.0
        return out

    @torch.no_grad()
    def fit_weights(self, data_loader, n_used=None, max_iters=1000, tol=1e-9, write=True):
        """All weights of the first ``n_used`` components at once, by EM with the components fixed (gbnf_weights_em): the
        fully-corrective step of boosting.  No reference counterpart; it supersedes ``update_rho``, which moves ``rho[component]``
        alone.  One pass over a loader of ``(x, _)``: every batch's component log-likelihoods go, in ONE flow launch, into their columns
        of a ``(n_used, rows)`` device table (sized by ``len(data_loader.dataset)`` when there is one; otherwise the batches' tables are
        concatenated once); then ONE library call iterates on that table, started at ``rho[:n_used] / sum``, until the mean
        log-likelihood moves by at most ``tol`` or ``max_iters`` updates were made -- no component forward and no host read per
        iteration.  ``write``: ``self.rho[:n_used]`` becomes ``w * sum(rho[:n_used])`` clamped to the reference's [0.01, 100] in place
        (gbnf_weights_to_rho; the entries beyond keep their standing).  Puts the module in eval mode.  ONE host read.  -> dict:
          nll_before, nll_after   -mean_i G(x_i) at the starting and at the final weights (never larger after than before)
          iters, converged        updates applied; whether the tolerance stopped them
          rows, excluded          rows used; rows left out (a NaN or +inf entry, or -inf under every component)
          weights                 the final w (n_used floats, before any clamp)
          clamped                 entries of rho that met the range (0 without ``write``)
        Default ``n_used`` as ``log_prob``.  An empty loader, or a rho with a negative or non-finite entry, raises ValueError."""
        self.eval()
        n_used = self._n_used(n_used)

        def batch_table(x, _, table, filled):
            for k in range(n_used):
                self._ensure_actnorm(x, k)
            self._guard(x, range(n_used))
            with torch.cuda.device(x.device):
                mix = self.native_mixture(n_used)
                if table is None:
                    return mix.component_log_prob(x, 0, n_used)
                mix.prepared_component_log_prob(x, table, 0, n_used, col_offset=filled)(native._stream_ptr())
        return self._fit_weights_over(data_loader, n_used, batch_table, max_iters, tol, write)

    # ---- the score: grad_x log p(x) of a component and of the mixture (gbnf_mixture_score), eval or train mode alike
    def _score_input(self, x, comps):
        self._require_device(x)
        x = x.detach().contiguous().float()
        if x.dim() != 2:
            raise ValueError(f"x must be (N, d), got {tuple(x.shape)}")
        for c in comps:
            if not all(bool(l.actnorm.inited) for l in getattr(getattr(self.flows[c], "flow", None), "layers", [])):
                raise ValueError("ActNorm not initiated: run a forward pass on data first (models/layers.py:473-475)")
        return x

    def _mixture_score(self, x, comps, log_w, ll, want_r):
        """One gbnf_mixture_score call on the trainers of ``comps``, on RUNNING statistics whatever the module's mode: the trainers'
        batch-statistics mode is switched off for the call and put back.  The call runs the trainers' forward, which re-derives the
        BatchNorm entries of their live blobs from the running statistics: a recorded train-mode forward of one of these components
        that still awaits its backward has lost the batch statistics its backward sweep reads there.  Like every other forward on
        a trainer, the call therefore moves ``forward_serial``, and that pending backward raises ``_FlowFunction``'s RuntimeError
        instead of returning wrong gradients (run the backward first, or the forward again)."""
        trainers = [self.native_trainer(c) for c in comps]
        modes = [t.batch_stats for t in trainers]
        try:
            for t in trainers:
                t.set_batch_stats(False)
                if t.has_batch_stats:
                    t.forward_serial = getattr(t, "forward_serial", 0) + 1
            return native.mixture_score(trainers, log_w, x, ll=ll, want_r=want_r)
        finally:
            for t, on in zip(trainers, modes):
                t.set_batch_stats(on)

    @torch.no_grad()
    def component_score(self, x, c):
        """-> (g_x (N,d), ll (N,)): the score grad_x ll_c(x) of component c and its log-density ll_c = log N(z_c;0,I) + ldj_c, from the
        training-path kernels on the live parameters with no weight gradient computed.  Running statistics in either module mode;
        nothing is recorded for autograd.  Uninitialised ActNorms raise ValueError as ``component_inverse``."""
        c = self._check_component(c)
        x = self._score_input(x, [c])
        with torch.cuda.device(x.device):
            g_x, ll, _ = self._mixture_score(x, [c], torch.zeros(1, dtype=torch.float32, device=x.device), None, False)
        return g_x, ll

    @torch.no_grad()
    def score(self, x, n_used=None, return_log_prob=False, return_responsibilities=False):
        """grad_x log p(x) of the mixture of the first ``n_used`` components (default as ``log_prob``), p = sum_c w_c p_c with
        w_c = rho_c / sum_{j < n_used} rho_j -- the closed form of ``log_prob``'s recursion -- as sum_c r_c grad_x ll_c with the
        responsibilities r_c = softmax_c(log w + ll).  The table ll is the evaluation path's (one launch for all components), so
        log_prob and responsibilities are its numbers; the gradient is ONE library call on the components' trainers.  In train()
        mode of a RealNVP with BatchNorm, ``score`` / ``component_score`` between a recorded forward of one of these components and
        its backward make that backward raise RuntimeError (the trainer's batch statistics are gone): finish the backward first.
        -> g_x (N,d), or (g_x[, log_prob (N,)][, responsibilities (N, C_used)])."""
        n_used = self._n_used(n_used)
        x = self._score_input(x, range(n_used))
        self._guard(x, range(n_used))
        with torch.cuda.device(x.device):
            ll = self.native_mixture(n_used).component_log_prob(x, 0, n_used)
            g_x, G, r = self._mixture_score(x, list(range(n_used)), self._log_w(n_used), ll, bool(return_responsibilities))
        return self._score_result(g_x, G, r, return_log_prob, return_responsibilities)

    @torch.no_grad()
    def responsibilities(self, x, n_used=None):
        """(N, C_used): p(component c | x) under the mixture ``score`` differentiates.  Needs no trainer: the evaluation path's table
        and gbnf_mixture_responsibilities."""
        n_used = self._n_used(n_used)
        x = self._score_input(x, range(n_used))
        self._guard(x, range(n_used))
        with torch.cuda.device(x.device):
            ll = self.native_mixture(n_used).component_log_prob(x, 0, n_used)
            r, _ = native.mixture_responsibilities(ll, self._log_w(n_used))
        return r.t()

    def boosting_weights(self, x, beta=1.0):
        """Step 1-2 of compute_kl_pq_loss (density_experiment.py:612-640) for training component ``self.component``:
        G = mixture log-density of the ``self.component`` FIXED components (recursion of :614-622), then
        w = softmax(-G), w^beta, clamp to [0.01, 0.1] when max(w) > 0.1, renormalise.  Returns (w (N,), G (N,)).
        The caller resamples with its own RNG: ``idx = torch.multinomial(w, N, replacement=True)`` (:642)."""
        if not (self.all_trained or self.component > 0):
            raise ValueError("the first component is trained without boosting weights (density_experiment.py:660-666)")
        G = self.log_prob(x, n_used=self.component)
        with torch.cuda.device(x.device):
            w = native.boosting_weights(G, beta)
        return w, G

    @staticmethod
    def check_numerics(reset=True):
        """Raise if any kernel since the last check met a split-f16 operand beyond the fp16 range (+-65504): inputs far
        outside the scale the flow was fitted on, or an exploding model.  The EVALUATION kernels
        repair such samples themselves (bf16x6 pass), so for them this is a data-quality alarm; the TRAINING kernels
        saturate there, so after a training epoch a non-zero count means wrong gradients.  Synchronises with the device;
        call it once per epoch, not per step."""
        n_train = native.training_saturation_count(reset=False)
        n = native.saturation_count(reset=reset)           # (the sum; resets both parts)
        if n:
            raise FloatingPointError(f"{n} wave(s) met a split-f16 operand beyond +-65504: {n - n_train} of evaluation launches (repaired on "
                                     f"the device), {n_train} of training launches (saturated: gradients of those samples are wrong) -- "
                                     "normalise the inputs")

    # ------------------------------------------------------------------ checkpoint side-car (fixes S5)
    def permutation_state(self):
        """What the reference's checkpoints lose: permutation indices, ActNorm ``inited``,
        ``component`` and ``all_trained`` -- and, for `--coupling_network random`, WHICH activation every coupling net
        drew at construction time (the state_dict of a TanhNet and of a ReLUNet look the same).  Save next to
        ``state_dict()``."""
        st = {"component": self.component, "all_trained": self.all_trained, "indices": {}, "actnorm_inited": {},
              "activations": [[list(a) if isinstance(a, tuple) else a for a in gspec.activation_pattern_of_component(f)]
                              for f in self.flows]}
        if self.component_type == "glow":
            for c, flow in enumerate(self.flows):
                for k, layer in enumerate(flow.flow.layers):
                    st["indices"][f"{c}.{k}"] = layer.permutation.indices.clone()
                    st["actnorm_inited"][f"{c}.{k}"] = bool(layer.actnorm.inited)
        return st

    def load_permutation_state(self, st):
        self.component = int(st["component"])
        self.all_trained = bool(st["all_trained"])
        if st.get("activations") is not None:
            self._set_activations(st["activations"])
        for name, idx in st["indices"].items():
            c, k = (int(v) for v in name.split("."))
            self.flows[c].flow.layers[k].permutation.set_indices(idx)
        for name, flag in st["actnorm_inited"].items():
            c, k = (int(v) for v in name.split("."))
            self.flows[c].flow.layers[k].actnorm.inited = bool(flag)

    def _set_activations(self, patterns):
        """Make every TanhNet / ReLUNet use the recorded activation (a model built with `--coupling_network random`
        draws them anew on every construction)."""
        changed = False
        for flow, pat in zip(self.flows, patterns):
            nets = ([layer.block for layer in flow.flow.layers] if self.component_type == "glow"
                    else [n for mods in flow.flow_param for n in (mods[0], mods[1])])
            acts = [a for step in pat for a in (step if isinstance(step, (list, tuple)) else [step])]
            for net, act in zip(nets, acts):
                if act == "residual" or not hasattr(net, "network"):
                    continue
                want = nn.Tanh if act == "tanh" else nn.ReLU
                for i, mod in enumerate(net.network):
                    if isinstance(mod, (nn.Tanh, nn.ReLU)) and not isinstance(mod, want):
                        net.network[i] = want()
                        changed = True
        if changed:                 # handles and trainers were built for the old architecture
            self._handles, self._handles_exact, self._trainers, self._mixture = {}, {}, {}, None
            self._per_step_act = None

    def load_spec(self, c, spec):
        """Install a flow spec's numbers (see spec.py) into component c's parameters."""
        flow = self.flows[c]
        dev = self.rho.device

        def put(dst, src):
            with torch.no_grad():
                dst.copy_(torch.as_tensor(np.asarray(src)).reshape(dst.shape).to(dev))

        def load_net(holder, net):
            linears = gspec.linears_of(holder)
            if len(linears) != len(net["layers"]):
                raise ValueError("coupling network depth mismatch")
            for m, (w, b) in zip(linears, net["layers"]):
                put(m.weight, w)
                put(m.bias, b)

        if spec["kind"] == "glow":
            for layer, st in zip(flow.flow.layers, spec["steps"]):
                put(layer.actnorm.bias, st["an_bias"])
                put(layer.actnorm.logs, st["an_logs"])
                layer.actnorm.inited = True
                layer.permutation.set_indices(st["perm"])
                load_net(layer.block, st["net"])
        else:
            for mods, st in zip(flow.flow_param, spec["steps"]):
                load_net(mods[0], st["t_net"])
                load_net(mods[1], st["s_net"])
                if st["bn"] is not None:
                    for key in ("log_gamma", "beta", "running_mean", "running_var"):
                        put(getattr(mods[2], key), st["bn"][key])
