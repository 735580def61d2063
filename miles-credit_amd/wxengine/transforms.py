"""Gen-2 variable transforms on the device: host mirrors of the reference's value-filling and variance-stabilising blocks.

Every WXFormer example under the reference's config/gen_2/examples that has a pre / post chain uses
    preblocks.per_step :  fill_values -> log_transform | sqrt_transform -> bridgescaler_transform(transform) -> concat
    postblocks.per_step:  reconstruct -> bridgescaler_transform(inverse_transform) -> exp_transform | square_transform -> ...

Input side -- DESCRIPTORS, not torch modules: `DevicePreblock(example, mean, std, transforms=[...])` compiles them into a per-channel
table and the fused kernel (csrc/wx_pre.h pre_xform_kernel) applies fill -> log | sqrt -> normalise -> concatenate in one pass.
    FillValues     credit/preblock/fill_values.py   (rules: search "nan" | number, op, fill; masks on the original value, last wins)
    LogTransform   credit/preblock/log.py           (log_base(x + eps) - log_base(eps), base "e" | "2" | "10")
    SqrtTransform  credit/preblock/sqrt.py
They take the reference's argument names and raise its errors.  Variable selection follows credit/preblock/_utils.py::
_parse_variable_selection (empty list = all, a partial path selects what lies beneath it, first-seen order, no duplicates), expanded
against the example input.  The kernel serves the canonical order fill* -> (log | sqrt)? -> scale -> concat per variable; anything
else -- a fill behind a log / sqrt, a second log / sqrt, more than 8 rules, a block whose data_types lack "input" -- is a ValueError
at construction, never a wrong result.  Stacked FillValues blocks on one variable are composed exactly (`compose_fill_rules`).

Output side -- post blocks, callables on the batch dict with the reference's `key` argument (csrc/wx_unxform.h):
    ExpTransform      credit/postblock/exp.py       base^(y + log_base(eps)) - eps
    SquareTransform   credit/postblock/square.py    y^2
    InverseTransforms(mean, std, blocks)            the inverse scale of `InverseScale` and the exp / square of every variable in ONE
                                                    launch; bit-identical to the chain InverseScale -> the single blocks
They read the views `Reconstruct` hands out where they lie and rebind the dict entry to a fresh tensor: y_pred is never modified.
No CPU fallback: construction raises without a GPU.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np

from .native import HandleCache, _check, _f32, _i32, _named_tensor_args, _stream_ptr, check_named_tensor, require_gpu
from .preblock import channel_stats

MAX_FILL_RULES = 8          # WX_MAX_FILL_RULES
MAX_VARIABLES = 64          # kMaxFields
VALID_DATA_TYPES = ("input", "target")
XFORM_NONE, XFORM_LOG_E, XFORM_LOG_2, XFORM_LOG_10, XFORM_SQRT = range(5)      # enum wx_xform
FILL_OPS = {"nan": 0, "==": 1, "!=": 2, "<": 3, "<=": 4, ">": 5, ">=": 6}      # enum wx_fill_op
_LOG_KIND = {"e": XFORM_LOG_E, "2": XFORM_LOG_2, "10": XFORM_LOG_10}
_NUMERIC_OPS = sorted(k for k in FILL_OPS if k != "nan")


def parse_variable_selection(variable_list: Sequence[str], state_dict: dict, data_types: Optional[Sequence[str]] = None) -> list:
    """credit/preblock/_utils.py::_parse_variable_selection: the full variable keys of `state_dict[data_type][source]` matched by
    `variable_list` (an entry matches itself and everything beneath it), in first-seen order without duplicates; empty = all."""
    if data_types is None:
        data_types = list(state_dict.keys())
    everything = []
    for dt in data_types:
        for source in state_dict.get(dt, {}).values():
            for name in source:
                if name not in everything:
                    everything.append(name)
    if not variable_list:
        return everything
    chosen = []
    for partial in variable_list:
        for name in everything:
            if (name == partial or name.startswith(partial + "/")) and name not in chosen:
                chosen.append(name)
    return chosen


def _check_data_types(data_types, note=""):
    data_types = list(data_types or VALID_DATA_TYPES)
    invalid = set(data_types) - set(VALID_DATA_TYPES)
    if invalid:
        raise ValueError(f"Invalid data_types {invalid}. Valid options are {VALID_DATA_TYPES}.{note}")
    return data_types


def _log_eps(base: str, eps: float, what: str) -> float:
    if base == "e":
        return math.log(eps)
    if base == "2":
        return math.log2(eps)
    if base == "10":
        return math.log10(eps)
    raise ValueError(f"Unsupported {what} '{base}'. Choose from: 'e', '2', '10'.")


class FillValues:
    """Descriptor of credit/preblock/fill_values.py::FillValues."""

    def __init__(self, rules: List[dict], variables: Optional[List[str]] = None, data_types: Optional[List[str]] = None):
        self.rules = rules
        self.variables = variables or []
        self.data_types = _check_data_types(data_types)
        for rule in rules:
            if "search" not in rule or "fill" not in rule:
                raise ValueError(f"Each rule must have 'search' and 'fill' keys, got: {rule}")
            if rule["search"] != "nan":
                if not isinstance(rule["search"], (int, float)):
                    raise ValueError(f"Rule 'search' must be 'nan' or a number, got: {rule['search']!r}")
                op = rule.get("op", "==")
                if op not in _NUMERIC_OPS:
                    raise ValueError(f"Rule 'op' must be one of {_NUMERIC_OPS}, got: {op!r}")

    def compiled_rules(self, dtype=np.float32):
        """[(op code, search, fill)] with search and fill rounded to `dtype`: float32 on the device, as comparing and torch.where
        against a float32 tensor round them (float64 serves the fp64 oracle of the tests)."""
        out = []
        for rule in self.rules:
            if rule["search"] == "nan":
                out.append((FILL_OPS["nan"], dtype(0.0), dtype(rule["fill"])))
            else:
                out.append((FILL_OPS[rule.get("op", "==")], dtype(rule["search"]), dtype(rule["fill"])))
        return out


class LogTransform:
    """Descriptor of credit/preblock/log.py::LogTransform."""

    def __init__(self, variables: List[str], data_types: Optional[List[str]] = None, base: str = "e", eps: float = 1e-8):
        self.variables = variables
        self.data_types = _check_data_types(data_types, " Preblocks never operate on 'metadata'.")
        self._eps = float(eps)
        self._log_eps = _log_eps(base, self._eps, "log base")
        self._base = base
        self.kind = _LOG_KIND[base]


class SqrtTransform:
    """Descriptor of credit/preblock/sqrt.py::SqrtTransform."""
    kind = XFORM_SQRT

    def __init__(self, variables: List[str], data_types: Optional[List[str]] = None):
        self.variables = variables
        self.data_types = _check_data_types(data_types, " Preblocks never operate on 'metadata'.")


def _rule_matches(op: int, x, search) -> bool:
    if op == 0:
        return bool(np.isnan(x))
    if np.isnan(x):
        return False
    return bool({1: x == search, 2: x != search, 3: x < search, 4: x <= search, 5: x > search, 6: x >= search}[op])


def apply_fill_rules(rules, x):
    """One FillValues block on one value (of the rules' dtype): every mask on `x` itself, the last matching rule wins."""
    out = x
    for op, search, fill in rules:
        if _rule_matches(op, x, search):
            out = fill
    return out


def compose_fill_rules(first, second):
    """The rule list, with every mask on the ORIGINAL value, that equals block `second` applied to the output of block `first`.
    Where `first` matched, its output is the constant fill, so `second` turns it into another constant; where it did not,
    `second` sees the original value.  Hence: the rules of `second` as they are, then the rules of `first` (which must win over
    them, in their own order) with each fill passed through `second`."""
    return list(second) + [(op, search, apply_fill_rules(second, fill)) for op, search, fill in first]


def compile_channel_table(transforms, example_input: Dict[str, Dict], keys: Sequence[str], levels: Sequence[int], dtype=np.float32):
    """-> None when no variable is touched, else dict of the per-output-channel arrays wx_pre_set_transforms takes: kind, eps,
    log_eps, n_rules [C]; rule_op, rule_search, rule_fill [C, 8].  `keys` / `levels`: the block's variables in channel order.
    `dtype`: float32 for the device; float64 keeps the constants unrounded for the tests' fp64 oracle."""
    per_var = {k: {"rules": [], "kind": XFORM_NONE, "eps": 1.0, "log_eps": 0.0} for k in keys}
    state = {"input": example_input}
    for blk in transforms or []:
        if not isinstance(blk, (FillValues, LogTransform, SqrtTransform)):
            raise ValueError(f"transforms takes FillValues, LogTransform and SqrtTransform descriptors, got {type(blk).__name__}")
        if "input" not in blk.data_types:
            raise ValueError(f"{type(blk).__name__}: data_types {blk.data_types} without 'input' -- the device preblock serves the input side only")
        for key in parse_variable_selection(blk.variables, state, blk.data_types):
            v = per_var[key]
            if isinstance(blk, FillValues):
                if v["kind"] != XFORM_NONE:
                    raise ValueError(f"{key}: fill_values behind a log / sqrt transform; the fused kernel serves fill* -> (log | sqrt)? -> scale")
                v["rules"] = compose_fill_rules(v["rules"], blk.compiled_rules(dtype))
                if len(v["rules"]) > MAX_FILL_RULES:
                    raise ValueError(f"{key}: {len(v['rules'])} fill rules, the fused kernel takes at most {MAX_FILL_RULES} per variable")
            else:
                if v["kind"] != XFORM_NONE:
                    raise ValueError(f"{key}: a second log / sqrt transform on one variable")
                v["kind"] = blk.kind
                if isinstance(blk, LogTransform):
                    v["eps"], v["log_eps"] = blk._eps, blk._log_eps
    if not any(v["rules"] or v["kind"] != XFORM_NONE for v in per_var.values()):
        return None
    nch = int(sum(levels))
    tab = dict(kind=np.zeros(nch, np.int32), eps=np.ones(nch, dtype), log_eps=np.zeros(nch, dtype),
               n_rules=np.zeros(nch, np.int32), rule_op=np.zeros((nch, MAX_FILL_RULES), np.int32),
               rule_search=np.zeros((nch, MAX_FILL_RULES), dtype), rule_fill=np.zeros((nch, MAX_FILL_RULES), dtype))
    cur = 0
    for k, nl in zip(keys, levels):
        v, sl = per_var[k], slice(cur, cur + nl)
        tab["kind"][sl], tab["eps"][sl], tab["log_eps"][sl] = v["kind"], dtype(v["eps"]), dtype(v["log_eps"])
        tab["n_rules"][sl] = len(v["rules"])
        for j, (op, search, fill) in enumerate(v["rules"]):
            tab["rule_op"][sl, j], tab["rule_search"][sl, j], tab["rule_fill"][sl, j] = op, search, fill
        cur += nl
    return tab


# ---- output side ---------------------------------------------------------------------------------------------------------------

class _Unxform:
    """One wx_unxform handle per (variables, shapes, device) signature, made on first use."""

    def __init__(self):
        self.lib = require_gpu("the device transforms have no CPU fallback")
        self._handles = HandleCache(self.lib, "wx_unxform")   # by signature

    def run(self, nested: Dict[str, Dict], plan):
        """plan: [(key, kind, eps, log_eps, mean or None, std or None)]; rebinds nested[source][key] to fresh tensors."""
        import torch
        if not plan:
            return
        if len(plan) > MAX_VARIABLES:
            raise ValueError(f"{len(plan)} variables in one launch, the kernel takes at most {MAX_VARIABLES}")
        ts = [nested[p[0].split("/")[0]][p[0]] for p in plan]
        t0 = ts[0]
        for p, t in zip(plan, ts):
            check_named_tensor(p[0], t, like=(plan[0][0], t0))
        B, _, nT, H, W = t0.shape
        dev = t0.device.index
        lv = [t.shape[1] for t in ts]

        def args():
            has = [p[4] is not None for p in plan]
            # per-(variable, level) statistics, keyed like the input side's: by the variable's short name
            named = [(p[0].split("/")[-1], p) for p in plan if p[4] is not None]
            mean, std = channel_stats([p[0] for p in plan], lv, {n: p[4] for n, p in named}, {n: p[5] for n, p in named})
            return (len(plan), _i32(lv), H, W, _i32([p[1] for p in plan]), _f32([p[2] for p in plan]), _f32([p[3] for p in plan]), _i32(has),
                    _f32(mean) if any(has) else None, _f32(std) if any(has) else None, dev)
        h = self._handles.get((tuple((p[0], n) for p, n in zip(plan, lv)), H, W, dev), args)
        src, bs, _, outs, dst = _named_tensor_args(ts)
        with torch.cuda.device(dev):
            _check(self.lib.wx_unxform_apply(h, src, bs, dst, B, nT, _stream_ptr(dev)))
        for p, o in zip(plan, outs):
            nested[p[0].split("/")[0]][p[0]] = o


class _PostTransform:
    kind = XFORM_NONE
    _eps, _log_eps = 1.0, 0.0

    def _setup(self, variables, key):
        self.variables = variables
        self.variables_expanded = False
        self.key = key
        self._dev = _Unxform()

    def expand(self, nested):
        """exp.py:74-80: lazily, against the first batch seen."""
        if not self.variables_expanded:
            self.variables = parse_variable_selection(self.variables, {"_": nested}, data_types=["_"])
            self.variables_expanded = True
        return self.variables

    def __call__(self, batch_dict: dict) -> dict:
        nested = batch_dict[self.key]
        plan = [(k, self.kind, self._eps, self._log_eps, None, None) for k in self.expand(nested)
                if k.split("/")[0] in nested and k in nested[k.split("/")[0]]]
        self._dev.run(nested, plan)
        return batch_dict

    forward = __call__


class ExpTransform(_PostTransform):
    """credit/postblock/exp.py::ExpTransform on the device; usable on its own behind `InverseScale`."""

    def __init__(self, variables: List[str], eps: float = 1e-8, base: str = "e", key: str = "y_processed"):
        self._eps = float(eps)
        self._log_eps = _log_eps(base, self._eps, "base")
        self._base = base
        self.kind = _LOG_KIND[base]
        self._setup(variables, key)


class SquareTransform(_PostTransform):
    """credit/postblock/square.py::SquareTransform on the device."""
    kind = XFORM_SQRT

    def __init__(self, variables: List[str], key: str = "y_processed"):
        self._setup(variables, key)


class InverseTransforms:
    """The fused post block: physical = normalised * std + mean (as `InverseScale`: variables without statistics skip it) and the
    exp / square of `blocks` for every variable of `batch_dict[key]` in one launch.  Variables with neither are passed through
    untouched (the same tensor object)."""

    def __init__(self, mean: Optional[Dict], std: Optional[Dict], blocks: Sequence[_PostTransform] = (), key: str = "y_processed"):
        self.mean, self.std, self.blocks, self.key = mean or {}, std or {}, list(blocks), key
        for blk in self.blocks:
            if not isinstance(blk, _PostTransform):
                raise ValueError(f"blocks takes ExpTransform and SquareTransform, got {type(blk).__name__}")
            if blk.key != key:
                raise ValueError(f"{type(blk).__name__} works on '{blk.key}', this block on '{key}'")
        self._dev = _Unxform()
        self._plan = None

    def __call__(self, batch_dict: dict) -> dict:
        nested = batch_dict[self.key]
        if self._plan is None:
            chosen = {}
            for blk in self.blocks:
                for k in blk.expand(nested):
                    if k in chosen:
                        raise ValueError(f"{k}: a second exp / square transform on one variable")
                    chosen[k] = blk
            plan = []
            for variables in nested.values():
                for k in variables:
                    name, blk = k.split("/")[-1], chosen.get(k)
                    if name not in self.mean and blk is None:
                        continue
                    plan.append((k, blk.kind if blk else XFORM_NONE, blk._eps if blk else 1.0, blk._log_eps if blk else 0.0,
                                 self.mean.get(name), self.std[name] if name in self.mean else None))
            self._plan = plan
        self._dev.run(nested, [p for p in self._plan if p[0].split("/")[0] in nested and p[0] in nested[p[0].split("/")[0]]])
        return batch_dict

    forward = __call__
