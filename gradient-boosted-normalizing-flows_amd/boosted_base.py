"""What the tabular ``BoostedFlow`` and the image ``BoostedImageFlow`` share: the reference's boosted-mixture bookkeeping
(models/boosted_flow.py: ``rho``, ``component``, ``all_trained``, the component draw, the rho loop, the un-normalised recursion) and the
host skeletons around the library calls that are the same for both.  Nothing here packs, keys or launches: that stays with the
subclasses, and so does everything on the per-call path of ``forward``."""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import native


# The three flag readers live here, not in boosted_flow.py, because the base reads ``deterministic`` and boosted_flow.py imports the
# base: the other way round would be an import cycle.  boosted_flow.py re-exports them, so ``boosted_flow.deterministic_from`` (and its
# two image siblings) remain the names callers, tests and the documents use.
def deterministic_from(args, env=None):
    """The deterministic-mode flag of a module: ``args.deterministic`` (a bool, or None / absent = not given), else the environment
    variable GBNF_DETERMINISTIC ("1" / "0"; unset or empty = off).  Anything else raises ValueError."""
    return _flag_from(args, env, "deterministic", "GBNF_DETERMINISTIC")


def image_deterministic_from(args, env=None):
    """The deterministic-mode flag of an IMAGE module's trainers (image_glow.BoostedImageFlow.image_deterministic):
    ``args.image_deterministic``, else the environment variable GBNF_IMAGE_DETERMINISTIC; the rules of ``deterministic_from``."""
    return _flag_from(args, env, "image_deterministic", "GBNF_IMAGE_DETERMINISTIC")


def image_eval_deterministic_from(args, env=None):
    """The deterministic-mode flag of an IMAGE module's evaluation handles (image_glow.BoostedImageFlow.image_eval_deterministic):
    ``args.image_eval_deterministic``, else the environment variable GBNF_IMAGE_EVAL_DETERMINISTIC; the rules of
    ``deterministic_from``.  A flag of its own: it reads neither of the other two and they do not read it."""
    return _flag_from(args, env, "image_eval_deterministic", "GBNF_IMAGE_EVAL_DETERMINISTIC")


def _flag_from(args, env, attr, var):
    given = getattr(args, attr, None)
    if given is not None:
        if not isinstance(given, (bool, int)) or given not in (0, 1, True, False):
            raise ValueError(f"{attr} must be a bool, got {given!r}")
        return bool(given)
    text = (os.environ if env is None else env).get(var, "")
    if text in ("", "0"):
        return False
    if text == "1":
        return True
    raise ValueError(f"{var} must be 0 or 1, got {text!r}")


class BoostedMixtureBase(nn.Module):
    """models/boosted_flow.py:BoostedFlow without its components: the subclass constructor appends ``flows`` and moves to the device."""

    _CACHES = ()                              # names in ``__dict__`` that hold tensor look-ups: dropped by ``_apply`` (.to / .cuda / .float)
    RHO_TOLERANCE, RHO_MIN_ITERS = 0.001, 10  # models/boosted_flow.py:158-160

    def __init__(self, args):
        super().__init__()
        self.args = args
        # bit-reproducible training steps: args.deterministic, else env GBNF_DETERMINISTIC, else off (what it switches is the subclass's)
        self.deterministic = deterministic_from(args)
        self.num_flows = args.num_flows
        self.z_size = args.z_size
        self.density_evaluation = args.density_evaluation
        self.all_trained = False
        self.component_type = args.component_type
        self.num_components = args.num_components
        self.component = 0
        # GenerativeFlow buffers (models/generative_flow.py:22-23): drawn before any component is constructed
        self.register_buffer("base_dist_mean", torch.randn(self.z_size).normal_(0, 0.1))
        self.register_buffer("base_dist_var", 3.0 * torch.ones(self.z_size))
        # rho (models/boosted_flow.py:32-39)
        if args.rho_init == "decreasing":
            rho = torch.clamp(1.0 / torch.pow(2.0, torch.arange(self.num_components * 1.0)), min=0.05)
        else:
            rho = torch.full((self.num_components,), 1.0 / self.num_components)
        self.register_buffer("rho", rho.float())
        self.flows = nn.ModuleList()
        self._handles = {}         # c -> (version key, evaluation handle)
        self._trainers = {}        # c -> (address key, trainer, ...)

    # ------------------------------------------------------------------ reference API
    def increment_component(self):
        """models/boosted_flow.py:52-59."""
        if self.component == self.num_components - 1:
            self.component = 0
            self.all_trained = True
        else:
            self.component = min(self.component + 1, self.num_components - 1)

    def _sample_component(self, sampling_components):
        """models/boosted_flow.py:61-96: "c" | "1:c" | "1:c-1" | "-c" -> component id (draws
        torch.multinomial over rho for the ranged forms)."""
        if sampling_components == "c":
            return min(self.component, self.num_components - 1)
        if sampling_components in ("1:c", "1:c-1"):
            if sampling_components == "1:c-1":
                n = self.component
            else:
                n = self.num_components if self.all_trained else self.component + 1
            n = min(max(n, 1), self.num_components)
            simplex = self.rho[0:n] / torch.sum(self.rho[0:n])
            return int(torch.multinomial(simplex, 1, replacement=True).item())
        if sampling_components == "-c":
            simplex = self.rho.clone().detach()
            simplex[self.component] = 0.0
            simplex = simplex / simplex.sum()
            return int(torch.multinomial(simplex, 1, replacement=True).item())
        raise ValueError("z_k can only be sampled from ['c', '1:c-1', '1:c', '-c'] "
                         "(corresponding to 'new', 'fixed', or new+fixed components)")

    # ------------------------------------------------------------------ argument checks
    def _n_used(self, n_used, default="trained"):
        """How many leading components a call looks at.  None: ``default`` -- "trained" = the components trained so far
        (``component + 1``, all of them once ``all_trained``), "all" = ``num_components``.  Anything outside [1, num_components] raises."""
        if n_used is None:
            if default not in ("trained", "all"):
                raise ValueError(f"default must be 'trained' or 'all', got {default!r}")
            n_used = self.num_components if default == "all" or self.all_trained else self.component + 1
        n_used = int(n_used)
        if not 1 <= n_used <= self.num_components:
            raise ValueError(f"n_used={n_used} outside [1, {self.num_components}]")
        return n_used

    def _require_device(self, x):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise native.GbnfError("x must live on the MI355X (cuda) device: this module has no CPU path")

    def _check_component(self, c):
        c = int(c)
        if not 0 <= c < self.num_components:
            raise ValueError(f"c={c} is no component of this model (0 .. {self.num_components - 1})")
        return c

    def _rho_in_place(self, what):
        """``self.rho`` for a library call that reads or writes it where it is; ``what``: the caller and what it does, for the refusal."""
        rho = self.rho
        if rho.dtype != torch.float32 or not rho.is_contiguous():
            raise ValueError(f"{what} self.rho in place: it must be contiguous float32")
        return rho

    def _log_w(self, n_used):
        rho = self.rho[:n_used].detach().float()
        return torch.log(rho / rho.sum()).contiguous()

    @staticmethod
    def _score_result(g_x, G, r, return_log_prob, return_responsibilities):
        out = (g_x,) + ((G,) if return_log_prob else ()) + ((r.t(),) if return_responsibilities else ())
        return out[0] if len(out) == 1 else out

    def _apply(self, fn, *a, **k):
        for name in self._CACHES:
            self.__dict__.pop(name, None)
        return super()._apply(fn, *a, **k)

    # ------------------------------------------------------------------ the mixture weights (models/boosted_flow.py:119-207)
    @staticmethod
    def _cycle(loader):
        """The loader's batches, over and over (a loader that yields nothing ends the generator)."""
        while True:
            empty = True
            for batch in loader:
                empty = False
                yield batch
            if empty:
                return

    def _rho_loop(self, data_loader, step_fn):
        """The loop of ``update_rho`` around one library call per iteration: ``step_fn(x, y, step_size)`` updates ``self.rho`` on the
        device and returns the call's 4 statistics (grad, rho before, rho after, |after - before|).  Nothing is read back up to
        iteration ``RHO_MIN_ITERS``, where the reference cannot stop, and the 4 statistics per iteration after that."""
        init_step, max_iters = self.args.rho_lr, self.args.rho_iters
        batches = self._cycle(data_loader)
        for batch_id in range(max_iters):
            (x, y) = next(batches)
            stats = step_fn(x, y, init_step / (0.05 * batch_id + 1))
            # the kernel wrote rho behind autograd's back: move its version counter as training_step does for parameters
            torch.autograd.graph.increment_version([self.rho])
            if batch_id > self.RHO_MIN_ITERS and (batch_id > max_iters or stats.tolist()[3] < self.RHO_TOLERANCE):
                break

    def _mixture_recursion(self, ll_columns):
        """models/boosted_flow.py:119-139 on the log-densities of components 0 .. ``self.component`` (one (n,) tensor each, taken one
        after the other) -> (new_ll, fixed_ll, full_ll).  Un-normalised rho, as in the reference, which starts all three at zeros
        (:120-122): with component == 0 (second boosting pass, all_trained) new_ll and fixed_ll stay zero, the gradient is 0 and rho[0]
        is left where it is."""
        new_ll = fixed_ll = full_ll = None
        for c, ll in enumerate(ll_columns):
            if c == 0:
                full_ll = ll
                fixed_ll = torch.zeros_like(ll)
                new_ll = torch.zeros_like(ll)
            else:
                new_ll = ll
                prev = torch.log(1 - self.rho[c]) + full_ll
                nxt = torch.log(self.rho[c]) + new_ll
                full_ll = torch.logsumexp(torch.stack([prev, nxt], dim=1), dim=1)
            if c == self.component - 1:
                fixed_ll = full_ll
        return new_ll, fixed_ll, full_ll

    def _fit_weights_over(self, data_loader, n_used, batch_table, max_iters, tol, write):
        """The pass of ``fit_weights`` over a loader of ``(x, y)``: the (n_used, rows) table of component log-likelihoods, then
        ``native.fit_weights_on_table``.  ``n_used``: checked by the caller (``_n_used``), whose hook needs it; the bound of the EM
        kernel is checked here.  ``batch_table(x, y, table, filled)`` is the subclass's part: with a ``table`` (the loader has
        a dataset, whose length sizes it) it writes the batch's (n_used, n) log-likelihoods into columns [filled, filled + n); with None
        it returns them, and the pieces are concatenated once."""
        if n_used > native.WEIGHTS_MAX_COMPONENTS:
            raise ValueError(f"fit_weights handles up to {native.WEIGHTS_MAX_COMPONENTS} components, got n_used = {n_used}")
        rho = self._rho_in_place("fit_weights reads (and with write=True writes)")
        dev = rho.device
        try:
            capacity = len(data_loader.dataset)
        except (AttributeError, TypeError):
            capacity = None
        table, filled, pieces = None, 0, []
        for (x, y) in data_loader:
            x = x.detach().to(dev)
            self._require_device(x)
            x = x.contiguous().float()
            if x.shape[0] == 0:
                continue
            if capacity is None:
                pieces.append(batch_table(x, y, None, filled))
            else:
                table = native.weights_table_room(table, n_used, capacity, filled, x.shape[0], dev)
                batch_table(x, y, table, filled)
            filled += x.shape[0]
        if filled == 0:
            raise ValueError("fit_weights: the loader yielded no rows")
        if capacity is None:
            table = pieces[0] if len(pieces) == 1 and pieces[0].is_contiguous() else torch.cat(pieces, dim=1)
        return native.fit_weights_on_table(table[:, :filled], rho, n_used, max_iters, tol, write)

    @staticmethod
    def _eval_sums(state):
        """The one host read of ``evaluate``: the device state (``native.eval_state``; None = no batch came) -> {name: value} in the
        names of ``native.EVAL_STATE``.  No rows: ValueError."""
        s = None if state is None else state.tolist()
        if s is None or s[0] == 0:
            raise ValueError("evaluate: the loader yielded no rows")
        return {name: s[k] for name, k in native.EVAL_STATE.items()}
