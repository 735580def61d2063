#!/usr/bin/env python
"""The route census: which kernels ONE forward launches, and how often, for every configuration / switch set that takes a different
branch of the engine's route decisions (Engine::plan_pair and gemm_route in csrc/wx_engine.hip).  Needs the GPU.

    python tools/make_route_census.py            # rewrites tests/golden/route_census.json

Per case: the engine is created under the case's environment, runs one warm-up forward, then one forward under profile(3); the
census is the sorted {kernel row: launches} of that forward ("class.sSTAGE@family") and the wx_query counters of QUERY_KEYS.  Names and
integers only.  The lat-band cases record rank 0's step of n virtual ranks; a band engine does not clear its counters between steps,
so theirs are the differences over the measured step (the two masks as they stand).

tests/test_route_census_gpu.py recomputes every case and requires equality with the fixture, exactly.  A pull request that moves
the route decisions without meaning to change one must pass it with the fixture untouched; one that changes a route ON PURPOSE
regenerates the fixture with this tool, deliberately, and says which rows moved and why."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(ROOT, "tests", "golden", "route_census.json")
for p in (os.path.join(ROOT, "miles-credit_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

QUERY_KEYS = ("launches", "split_gemms", "gemm8p_launches", "splitk_gemms", "attn_blk", "attn_nkf_mask", "attn_block_nkf_mask",
              "ff_split_fused", "ff_split_pre", "ff_split_post")
MASK_KEYS = ("attn_nkf_mask", "attn_block_nkf_mask")

# the six bf16 switch sets of tests/test_teacher_forced_gpu.ROUTES, on the configurations it runs them on
PLAIN = {"WX_ATTN_BLOCK": "0", "WX_NO_FFFUSE": "1", "WX_NO_STREAM": "1", "WX_NO_WREG": "1"}
ROUTES = {
    "plain": (PLAIN, ("T1", "C1", "T5")),
    "ff_fused": ({"WX_FF_MIN_WGS": "0", "WX_ATTN_BLOCK": "0"}, ("T1", "C1")),
    "default": ({}, ("T1", "C1")),
    "attn_block": ({"WX_ATTN_BLOCK": "1"}, ("T1", "T5", "RT")),
    "stream": ({"WX_STREAM_MIN_ROWS": "0"}, ("T5", "C1")),      # T5: the only small case on KBlk::attn and KBlk::hidden
    "wreg": ({"WX_WREG_MIN_ROWS": "0", "WX_SKINNY_MAX": "0"}, ("T5", "C1")),
}


def _case(prec, name, tag="default", env=None, debug=0, ranks=0):
    return dict(id=f"{prec}-{name}-{tag}", prec=prec, config=name, env=dict(env or {}), debug=debug, ranks=ranks)


CASES = [_case("bf16", n, r, env) for r, (env, names) in ROUTES.items() for n in names] + [
    _case("bf16", "C1", "debug1", debug=1), _case("bf16", "C1", "debug2", debug=2),    # level 1 flips pre / post / attn_kblk
    _case("bf16", "T0H"), _case("bf16", "T1H"),                                        # dim_head 64 / 128: every dim_head == 32 term false
    _case("fp32s", "C1"), _case("fp32s", "C1", "no_pre", {"WX_NO_FF_SPLIT_PRE": "1"}),
    _case("fp32s", "C1", "no_post", {"WX_NO_FF_SPLIT_POST": "1"}), _case("fp32s", "C1", "no_256", {"WX_NO_FF_SPLIT_256": "1"}),
    _case("fp32", "T1"), _case("fp32s", "T1"),                                         # fp32: the chain everywhere
    _case("bf16", "T1", "band2", ranks=2), _case("fp32s", "T1", "band3", ranks=3),     # the smallest splits of test_latband_gpu
]


def _queries(eng):
    return {k: eng.query(k) for k in QUERY_KEYS}


def census(case):
    """-> {"kernels": {row: launches}, "queries": {key: value}} of one forward of `case` (an entry of CASES)."""
    import torch
    from wxengine.config import named_config
    from wxengine.engine import WXEngine
    from wxengine.latband import VirtualBands
    from wxengine.synth import synth_input, synth_state_dict

    env = case["env"]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:    # the switches are read when an engine is created
        cfg = named_config(case["config"])
        sd = synth_state_dict(cfg)
        if case["ranks"]:
            vb = VirtualBands(cfg, sd, case["ranks"], case["prec"])
            eng, run = vb.ranks[0].eng, vb.step
        else:
            eng = WXEngine(cfg, case["prec"], 0)
            eng.load_state_dict(sd)
            eng.finalize()
            run = eng.forward
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    x = torch.from_numpy(synth_input(cfg)).cuda()
    eng.set_debug(case["debug"])
    run(x)
    torch.cuda.synchronize()
    before = _queries(eng)
    eng.profile(3)
    eng.profile_reset()
    run(x)
    torch.cuda.synchronize()
    kernels = {r["name"]: int(r["launches"]) for r in eng.profile_read()}
    eng.profile(0)
    q = _queries(eng)
    if case["ranks"]:
        q = {k: v if k in MASK_KEYS else v - before[k] for k, v in q.items()}
    return {"kernels": dict(sorted(kernels.items())), "queries": q}


def main():
    out = {}
    for case in CASES:
        out[case["id"]] = census(case)
        print(f"[census] {case['id']}: {len(out[case['id']]['kernels'])} rows, {out[case['id']]['queries']['launches']} launches", flush=True)
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
