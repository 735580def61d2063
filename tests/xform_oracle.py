"""A torch restatement of the two transform kernels (csrc/wx_pre.h pre_xform_kernel, csrc/wx_unxform.h) in the precision asked for,
working from the SAME compiled channel table the device gets (wxengine.transforms.compile_channel_table: stacked FillValues blocks
composed into one rule list whose masks all look at the original value).  tests/test_xform_oracle.py pins it to the goldens the
reference's own classes produced, tests/test_xform_vs_reference.py to the live classes; oracle/ is frozen, so it lives here."""
import numpy as np
import torch

from xform_cases import XFORM_CASES, batch_input, case_stats, out_variables, post_blocks, pre_blocks, target_channel_map


def _np_dtype(dtype):
    return np.float64 if dtype == torch.float64 else np.float32


def fill(x, ops, search, fills):
    """The kernel's rule loop on a tensor: every mask on the original `x`, applied in order."""
    nan = torch.isnan(x)
    out = x
    for op, s, f in zip(ops, search, fills):
        s = torch.tensor(s, dtype=x.dtype)
        mask = nan if op == 0 else ~nan & {1: torch.eq, 2: torch.ne, 3: torch.lt, 4: torch.le, 5: torch.gt, 6: torch.ge}[int(op)](x, s)
        out = torch.where(mask, torch.tensor(f, dtype=x.dtype), out)
    return out


def forward(x, kind, eps, log_eps):
    if kind == 0:
        return x
    if kind == 4:
        return torch.sqrt(x)
    log = {1: torch.log, 2: torch.log2, 3: torch.log10}[int(kind)]
    return log(x + torch.tensor(eps, dtype=x.dtype)) - torch.tensor(log_eps, dtype=x.dtype)


def inverse(p, kind, eps, log_eps):
    if kind == 0:
        return p
    if kind == 4:
        return p * p
    q = p + torch.tensor(log_eps, dtype=p.dtype)
    e = {1: torch.exp, 2: torch.exp2, 3: lambda t: torch.pow(10.0, t)}[int(kind)](q)
    return e - torch.tensor(eps, dtype=p.dtype)


def _stat(a, dtype):
    return torch.as_tensor(np.asarray(a, np.float32)).to(dtype).reshape(1, -1, 1, 1, 1)


def pre_variables(transforms, fields, mean, std, dtype, skip=()):
    """{source: {key: float32 array}} physical -> {key: tensor [B, n_levels, T, H, W]} filled, transformed and normalised.
    `skip`: stages left out ("fill", "xf", "rule<k>": the k-th compiled rule of every variable) -- the power test's knob."""
    from wxengine.transforms import compile_channel_table
    flat = {k: v for src in fields.values() for k, v in src.items()}
    keys, levels = list(flat), [flat[k].shape[1] for k in flat]
    tab = compile_channel_table(transforms, fields, keys, levels, dtype=_np_dtype(dtype))
    out, cur = {}, 0
    for k, nl in zip(keys, levels):
        x = torch.from_numpy(np.asarray(flat[k])).to(dtype)
        if tab is not None:
            n = int(tab["n_rules"][cur])
            use = [j for j in range(n) if f"rule{j}" not in skip and "fill" not in skip]
            x = fill(x, tab["rule_op"][cur][use], tab["rule_search"][cur][use], tab["rule_fill"][cur][use])
            if "xf" not in skip:
                x = forward(x, tab["kind"][cur], tab["eps"][cur], tab["log_eps"][cur])
        name = k.split("/")[-1]
        if mean is not None and name in mean:
            x = (x - _stat(mean[name], dtype)) / _stat(std[name], dtype).clamp(min=1e-12)
        out[k] = x
        cur += nl
    return out


def post_named(y_pred, cmap, mean, std, xf, dtype, skip=()):
    """y_pred [B, C_out, T, H, W] normalised -> {key: tensor} physical: the slices of `cmap` (the target channel map), the inverse
    scale of the variables that have statistics, then exp / square where xf[key] = ("log", base, eps) | ("sqrt",) says so."""
    import math
    y = torch.from_numpy(np.asarray(y_pred)).to(dtype).flatten(1, 2)
    npd, out = _np_dtype(dtype), {}
    for key, info in cmap.items():
        n = key.split("/")[-1]
        p = y[:, info["slice"]].unflatten(1, tuple(info["orig_shape"]))
        if mean is not None and n in mean and "scale" not in skip:
            p = p * _stat(std[n], dtype) + _stat(mean[n], dtype)
        t = xf.get(key)
        if t and "xf" not in skip:
            if t[0] == "log":
                eps = float(t[2])
                log_eps = {"e": math.log, "2": math.log2, "10": math.log10}[t[1]](eps)
                p = inverse(p, {"e": 1, "2": 2, "10": 3}[t[1]], npd(eps), npd(log_eps))
            else:
                p = inverse(p, 4, 0.0, 0.0)
        out[key] = p
    return out


def post_variables(name, y_pred, dtype, skip=()):
    mean, std = case_stats(name)
    return post_named(y_pred, target_channel_map(name), mean, std, {v["key"]: v["xf"] for v in out_variables(name)}, dtype, skip)


def case_outputs(name, fields, y_pred, dtype, skip=()):
    """-> {"pre:<var>": array, "post:<var>": array} of one case, the names of the fixtures."""
    import wxengine.transforms as X
    mean, std = case_stats(name)
    pre = pre_variables(pre_blocks(name, X), batch_input(name, fields), mean, std, dtype, skip)
    post = post_variables(name, y_pred, dtype, skip)
    out = {f"pre:{v['name']}": pre[v["key"]].numpy() for v in XFORM_CASES[name]["variables"]}
    out.update({f"post:{v['name']}": post[v["key"]].numpy() for v in out_variables(name)})
    return out
