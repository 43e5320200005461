"""Fused flat-bucket optimizers with the surface the reference's training driver calls (train.py:100-164):

    optimizer = subgc.optim.build_optimizer(model, opt)                   # misc/utils.py:223-239 (train.py:100)
    optimizer.load_state_dict(torch.load(.../optimizer.pth))              # train.py:102
    utils.set_lr(optimizer, lr)                                           # misc/utils.py:158-160 (train.py:110,122)
    optimizer.zero_grad(); loss.backward()                                # train.py:150,161
    optimizer.step()                                                      # the clip of train.py:163 is IN the sweep
    torch.save(optimizer.state_dict(), .../optimizer.pth)                 # train.py:47

Every `--optim` rule (adam, adamw, sgd, sgdm, sgdmom, rmsprop, adagrad) runs as ONE fused sweep over the model's flat buffers
(subgc_clip_optim_step): global-norm clip (misc/utils.py:174-200), the torch class's update, the bf16 weight snapshot, optionally
the next iteration's zero_grad.  `param_groups`, `state_dict()` and `load_state_dict()` use exactly the format of the torch class
built over the REFERENCE's `parameters()` order, so optimizer.pth files move between the reference and this package both ways.

Parameters whose reference gradient is None for the model's configuration (dead GCN units, an unused predicate embedding) are
skipped as torch skips them: no decay, no state, no step count (`skipped_param_names`).
"""
from __future__ import annotations

import torch

from . import ops

# top-level modules in the order the reference registers them: AttModel.__init__ (models/AttModel.py:72-120), then TopDownModel's
# `core` (:480).  The flat buffer orders the decoder differently (AttModel._specs: readiness order of the backward).
_REF_MODULES = ("obj_v_proj", "sg_obj_embed", "obj_emb_proj", "sg_pred_embed", "pred_emb_prj", "gcn_backbone", "gpn_layer", "read_out_proj",
                "logit", "embed", "fc_embed", "att_embed", "ctx2att", "core")

_CLASSES = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "sgd": torch.optim.SGD, "rmsprop": torch.optim.RMSprop,
            "adagrad": torch.optim.Adagrad}
_STATE_KEYS = {"adam": ("exp_avg", "exp_avg_sq"), "adamw": ("exp_avg", "exp_avg_sq"), "sgd": ("momentum_buffer",), "rmsprop": ("square_avg",),
               "adagrad": ("sum",)}


def reference_param_names(model):
    """Parameter names in the reference's `model.parameters()` order (its module registration order), for any preset."""
    names = [n for n, _ in model.named_parameters()]
    unknown = [n for n in names if n.split(".")[0] not in _REF_MODULES]
    if unknown:
        raise ValueError(f"parameters outside the reference's module tree: {unknown}")
    return sorted(names, key=lambda n: _REF_MODULES.index(n.split(".")[0]))          # stable: module-internal order is the reference's


def skipped_param_names(model):
    """Parameters the reference leaves WITHOUT a gradient (.grad None) for the model's configuration, in reference order: the GCN units
    whose outputs never reach the loss (AttModel._gcn_liveness; units 0-1 of a layer update the nodes, 2-3 the edges) and the predicate
    embedding when no live unit reads the edge features.  torch.optim skips them; so does the fused sweep."""
    needX, needP, live_nodes, live_edges = model._gcn_liveness()
    names = reference_param_names(model)
    dead = set()
    if not needP[0]:
        dead |= {"sg_pred_embed.weight", "pred_emb_prj.weight", "pred_emb_prj.bias"}
    for l in range(model.GCN_layers):
        for u in range(4):
            if not (live_nodes[l] if u < 2 else live_edges[l]):
                pre = f"gcn_backbone.gcn.{l}.gcn_collect.collect_units.{u}."
                dead |= {n for n in names if n.startswith(pre)}
    return [n for n in names if n in dead]


def _rekey(sd, perm):
    groups = sd["param_groups"]
    if len(groups) != 1 or len(groups[0]["params"]) != len(perm):
        raise ValueError(f"re-keying needs ONE parameter group over all {len(perm)} parameters of the model")
    pos = {pid: k for k, pid in enumerate(groups[0]["params"])}
    group = dict(groups[0], params=list(range(len(perm))))
    if "param_names" in groups[0]:
        names = [None] * len(perm)
        for k, nm in enumerate(groups[0]["param_names"]):
            names[perm[k]] = nm
        group["param_names"] = names
    return {"state": {perm[pos[pid]]: v for pid, v in sd["state"].items()}, "param_groups": [group]}


def _perm(model):
    ref = {n: j for j, n in enumerate(reference_param_names(model))}
    return [ref[n] for n, _ in model.named_parameters()]


def state_dict_to_reference(model, sd):
    """A torch optimizer's state_dict saved over `model.parameters()` (this package's order) -> the same state keyed in the reference's
    order, as the reference's own optimizer.pth (and the fused optimizer) expect it."""
    return _rekey(sd, _perm(model))


def state_dict_from_reference(model, sd):
    """The inverse: a reference optimizer.pth -> keyed for a torch optimizer built over `model.parameters()`."""
    perm = _perm(model)
    inv = [0] * len(perm)
    for i, j in enumerate(perm):
        inv[j] = i
    return _rekey(sd, inv)


def _step_count(v):
    x = float(v.item() if torch.is_tensor(v) else v)       # a tensor since torch 1.12, an int before (the reference's torch)
    if x < 0 or x != int(x):
        raise ValueError(f"bad optimizer step count {v!r}")
    return int(x)


class FusedOptimizer:
    """One torch.optim rule ('adam', 'adamw', 'sgd', 'rmsprop', 'adagrad'; hyperparameters as the torch class takes them) with the
    global-norm clip, over the model's flat buffers.  `fold_zero_grad`: the default of step(zero_grad=...), which leaves the gradient
    bucket zeroed by the sweep itself so that the next zero_grad() costs nothing (then the clipped gradients are not readable after the
    step, as they are under torch).  `skip_dead=False` sweeps the whole bucket: no parameter is skipped (parallel.FlatAdam)."""

    def __init__(self, model, kind, clip_norm=10.0, fold_zero_grad=False, skip_dead=True, **hyper):
        if kind not in _CLASSES:
            raise ValueError(f"unknown optimizer {kind!r} (one of {sorted(_CLASSES)})")
        probe = _CLASSES[kind]([torch.zeros(1, requires_grad=True)], **hyper)       # torch validates and fills in its defaults
        self.model, self.kind, self.clip_norm, self.fold_zero_grad = model, kind, clip_norm, fold_zero_grad
        self.defaults = dict(probe.defaults)
        self.names = reference_param_names(model)
        self.skipped = frozenset(skipped_param_names(model) if skip_dead else ())
        self.param_groups = [dict({k: v for k, v in probe.param_groups[0].items() if k != "params"}, params=[model.P(n) for n in self.names])]
        self._rule(self.param_groups[0])
        fp = model.flat_params
        self._s1 = torch.zeros_like(fp)
        self._s2 = torch.zeros_like(fp) if kind in ("adam", "adamw") else None
        if kind == "adagrad" and self.param_groups[0]["initial_accumulator_value"] != 0:
            self._s1.fill_(float(self.param_groups[0]["initial_accumulator_value"]))
        self.sumsq = torch.zeros(1, device=fp.device)
        self._live = self._live_table()
        self.t = 0                     # steps taken by the live parameters (they share one count)
        self._started = False          # SGD: the momentum buffers exist (torch initialises them with the first step's gradient)
        self._skipped_state = {}       # state entries of skipped parameters read from a file: saved again as they are
        self.reducer = None            # a GradBucketReducer(optimizer=self) accumulates the clip norm slice by slice (begin_step / accumulate)
        self._have = None

    # ------------------------------------------------------------------ plumbing
    def _live_table(self):
        """[lo, hi) element ranges of the live parameters in the flat buffer (slots and their 8-element padding, adjacent ones merged) as
        an int64 device tensor; None when nothing is skipped."""
        if not self.skipped:
            return None
        m, ranges = self.model, []
        for name, _ in sorted(m._slots.items(), key=lambda kv: kv[1][0]):
            if name in self.skipped:
                continue
            o, n, _ = m._slots[name]
            lo, hi = o, o + (n + 7) // 8 * 8
            if ranges and ranges[-1][1] == lo:
                ranges[-1][1] = hi
            else:
                ranges.append([lo, hi])
        flat = [x for r in ranges for x in r]
        return torch.tensor(flat, dtype=torch.int64).to(m.flat_params.device)

    def _slot(self, buf, name):
        o, n, shape = self.model._slots[name]
        return buf[o:o + n].view(shape)

    def _rule(self, g):
        """-> (sweep rule, h0, h1, eps, nesterov) of a parameter group; options the sweep does not implement raise."""
        if g.get("maximize", False):
            raise NotImplementedError("maximize=True is not supported by the fused sweep")
        if self.kind in ("adam", "adamw"):
            if g.get("amsgrad", False):
                raise NotImplementedError("amsgrad=True is not supported by the fused sweep")
            decoupled = self.kind == "adamw" or g.get("decoupled_weight_decay", False)
            return ("adamw" if decoupled else "adam"), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), False
        if self.kind == "sgd":
            return "sgd", float(g["momentum"]), float(g["dampening"]), 0.0, bool(g["nesterov"])
        if self.kind == "rmsprop":
            if g.get("momentum", 0) != 0 or g.get("centered", False):
                raise NotImplementedError("RMSprop with momentum or centered=True is not supported by the fused sweep")
            return "rmsprop", float(g["alpha"]), 0.0, float(g["eps"]), False
        return "adagrad", float(g["lr_decay"]), 0.0, float(g["eps"]), False

    def _check_grads(self):
        m = self.model
        fg = m.flat_grads
        if fg is None or fg.device != m.flat_params.device:
            raise RuntimeError("no gradient bucket: call optimizer.zero_grad() (model.flatten_grads()) before the forward")
        if self._s1.device != fg.device:
            raise RuntimeError(f"optimizer state on {self._s1.device}, model on {fg.device}: build the optimizer after moving the model")
        views = m.__dict__.get("_grad_views")
        for name, p in m._pmap.items():
            if views is None or p.grad is not views.get(name):
                raise RuntimeError(f"{name}.grad is not a view of the flat gradient bucket, so this step's gradients are not in "
                                   "model.flat_grads: call optimizer.zero_grad() before the forward instead of setting .grad to None")

    def begin_step(self):
        """(reducer.prepare) a new set of gradients: the norm accumulator starts from zero."""
        ops.fill_(self.sumsq, 0.0)
        self._have = set()

    def accumulate(self, stage, lo, hi):
        """sumsq += |flat_grads[lo:hi]|^2 on the CURRENT stream (the slice is final -- and, with several ranks, reduced -- there)."""
        if self._have is None or stage in self._have:
            return
        self._have.add(stage)
        ops.sumsq(self.model.flat_grads[lo:hi], self.sumsq)

    # ------------------------------------------------------------------ torch.optim surface
    def zero_grad(self, set_to_none=True):
        """Every .grad becomes (stays) a view of the zeroed flat bucket (model.flatten_grads) -- never None: the fused step reads the
        bucket.  Free after a step that folded the zeroing in."""
        self.model.flatten_grads()

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0, zero_grad=None):
        """Clip + update from the flat gradient bucket, with the hyperparameters currently in `param_groups[0]` (set_lr works).
        `grad_scale`: 1 / world after a SUM all-reduce (GradBucketReducer.finish(average=False)).  `zero_grad`: leave the bucket zeroed
        (default: the constructor's `fold_zero_grad`)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        m = self.model
        self._check_grads()
        g = self.param_groups[0]
        rule, h0, h1, eps, nesterov = self._rule(g)
        if self._have:                                          # some slices are in already: add whatever was not announced early
            for st, lo, hi in self.reducer.buckets:
                if hi > lo:
                    self.accumulate(st, lo, hi)
            self._have = None
        else:                                                   # nothing accumulated (one rank, or no reducer): one pass over the bucket
            self._have = None
            ops.fill_(self.sumsq, 0.0)
            ops.sumsq(m.flat_grads, self.sumsq)
        zero = self.fold_zero_grad if zero_grad is None else bool(zero_grad)
        snap = m.weights_b16() if getattr(m, "bf16_storage", False) else None     # compute_dtype = bf16: refreshed in the same sweep
        t = self.t + 1
        ops.clip_optim_step(rule, m.flat_params, m.flat_grads, self._s1, self._s2, self._live, self.sumsq, self.clip_norm, grad_scale,
                            g["lr"], h0, h1, eps, g["weight_decay"], t, nesterov=nesterov, first=not self._started, p_bf16=snap,
                            zero_grad=zero)
        self.t = t
        if rule == "sgd" and h0 != 0:
            self._started = True
        m.__dict__["_grads_are_zero"] = (m.flat_grads.data_ptr(), m.flat_grads._version, ops.GRAD_WRITES[0]) if zero else None
        # the kernel wrote the weights through raw pointers: the decode-time snapshots must be told explicitly
        m.invalidate_decode_caches()
        if snap is not None:
            m.weights_b16(fresh_from_optimizer=True)
        return loss

    def state_dict(self):
        """torch.optim.<class>.state_dict() of the same run, keyed in the reference's parameter order."""
        g = self.param_groups[0]
        keys = _STATE_KEYS[self.kind]
        state = {}
        for i, name in enumerate(self.names):
            if name in self.skipped:
                if i in self._skipped_state:
                    state[i] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in self._skipped_state[i].items()}
                elif self.kind == "adagrad":                    # Adagrad creates every parameter's state up front
                    state[i] = {"step": torch.tensor(0.0), "sum": self._slot(self._s1, name).clone()}
                continue
            if self.kind == "sgd":
                if self._started:
                    state[i] = {"momentum_buffer": self._slot(self._s1, name).clone()}
                continue
            if self.t == 0 and self.kind != "adagrad":          # the other classes create it lazily, at the first step
                continue
            e = {"step": torch.tensor(float(self.t))}
            for k, buf in zip(keys, (self._s1, self._s2)):
                e[k] = self._slot(buf, name).clone()
            state[i] = e
        group = dict({k: v for k, v in g.items() if k != "params"}, params=list(range(len(self.names))))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, state_dict):
        """Load a state_dict of the matching torch class (saved over the reference's parameter order, by the reference, by torch or by
        this class).  The group hyperparameters come from the file, as in torch.  The live parameters must share one step count."""
        groups = state_dict["param_groups"]
        N = len(self.names)
        if len(groups) != 1 or len(groups[0]["params"]) != N:
            raise ValueError(f"expected one parameter group over {N} parameters in the reference's order (a file saved by a torch optimizer "
                             "over model.parameters() is re-keyed by subgc.optim.state_dict_to_reference)")
        pos = {pid: k for k, pid in enumerate(groups[0]["params"])}
        st = {pos[pid]: v for pid, v in state_dict["state"].items()}
        cur = self.param_groups[0]
        grp = {k: v for k, v in cur.items() if k != "params"}
        grp.update({k: v for k, v in groups[0].items() if k not in ("params", "param_names")})
        grp["params"] = cur["params"]
        self._rule(grp)
        keys = _STATE_KEYS[self.kind]
        live = [i for i, n in enumerate(self.names) if n not in self.skipped]
        has = lambda e: all(e.get(k) is not None for k in keys)
        present = [i for i in live if i in st and has(st[i])]
        if present and len(present) != len(live):
            miss = [self.names[i] for i in live if i not in present]
            raise ValueError(f"optimizer state for {len(present)} of {len(live)} live parameters (none for {miss[:3]}...): the fused optimizer "
                             "keeps ONE step count for all of them")
        if self.kind == "adagrad" and not present:
            raise ValueError("an Adagrad state_dict holds every parameter's state; this one has none")
        t = 0
        if self.kind != "sgd":
            steps = sorted({_step_count(st[i]["step"]) for i in present})
            if len(steps) > 1:
                raise ValueError(f"the live parameters carry different step counts {steps}: the fused optimizer keeps one for all of them")
            t = steps[0] if steps else 0
        elif present:
            t = 1
        for i, name in enumerate(self.names):
            if i not in present:
                continue
            for k, buf in zip(keys, (self._s1, self._s2)):
                dst, src = self._slot(buf, name), st[i][k]
                if src.numel() != dst.numel():
                    raise ValueError(f"state {k!r} of {name}: {tuple(src.shape)} against the parameter's {tuple(dst.shape)}")
        if not present:
            self._s1.zero_()
            if self._s2 is not None:
                self._s2.zero_()
        for i in present:
            for k, buf in zip(keys, (self._s1, self._s2)):
                self._slot(buf, self.names[i]).copy_(st[i][k].reshape(self._slot(buf, self.names[i]).shape))
        self._skipped_state = {i: {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in st[i].items()}
                               for i, n in enumerate(self.names) if n in self.skipped and i in st}
        self.t, self._started = t, bool(present) and self.kind == "sgd"
        cur.clear()
        cur.update(grp)
        m = self.model
        m.invalidate_decode_caches()
        if getattr(m, "bf16_storage", False):
            m.weights_b16()


def build_optimizer(model, opt, clip_norm=10.0, fold_zero_grad=False):
    """misc/utils.py:223-239 over the model's flat buffers: same `opt.optim` names, same hyperparameters, same error.  The global-norm
    clip of train.py:163 (misc/utils.py:174-200, clip_norm 10) is part of every step."""
    lr = opt.learning_rate
    kw = dict(clip_norm=clip_norm, fold_zero_grad=fold_zero_grad)
    if opt.optim == "rmsprop":
        return FusedOptimizer(model, "rmsprop", lr=lr, alpha=opt.optim_alpha, eps=opt.optim_epsilon, weight_decay=opt.weight_decay, **kw)
    elif opt.optim == "adagrad":
        return FusedOptimizer(model, "adagrad", lr=lr, weight_decay=opt.weight_decay, **kw)
    elif opt.optim == "sgd":
        return FusedOptimizer(model, "sgd", lr=lr, weight_decay=5e-4, momentum=0.9, **kw)
    elif opt.optim == "sgdm":
        return FusedOptimizer(model, "sgd", lr=lr, momentum=opt.optim_alpha, weight_decay=opt.weight_decay, **kw)
    elif opt.optim == "sgdmom":
        return FusedOptimizer(model, "sgd", lr=lr, momentum=opt.optim_alpha, weight_decay=opt.weight_decay, nesterov=True, **kw)
    elif opt.optim == "adam":
        return FusedOptimizer(model, "adam", lr=lr, betas=(opt.optim_alpha, opt.optim_beta), eps=opt.optim_epsilon,
                              weight_decay=opt.weight_decay, **kw)
    elif opt.optim == "adamw":
        return FusedOptimizer(model, "adamw", lr=lr, weight_decay=0.01, **kw)
    else:
        raise Exception("bad option opt.optim: {}".format(opt.optim))
