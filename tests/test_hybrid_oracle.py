"""tests/hybrid_oracle.py (the plain-torch restatement of credit/postblock/hybrid_interp.py) against the reference's goldens
(tests/golden/hybrid_*.npz, written by tools/make_goldens.py --only hybrid): every variable of every case within 1e-6 of the fp32
golden in fp32 and within 1e-12 of the fp64 golden in fp64 (distance max |a - b| / max |b|; the fp64 golden is stored as a float32
difference, whose own rounding is allowed for element by element).  Then the conditions the cases are there for, and the mutations
of the restatement that the goldens must catch.  Needs neither a GPU nor the reference."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import hybrid_oracle as HO  # noqa: E402
from hybrid_cases import (HYBRID_CASES, case_inputs, check_conditions, distance, gate, load_golden, midpoints, raw_coefficients,  # noqa: E402
                          variables)

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def run_oracle(name, inp, dtype, mutation=None):
    if mutation in HO.COEFFICIENT_MUTATIONS:
        r = raw_coefficients(name)
        coef = (HO.midpoint_coefficients(r["source_a"], r["source_b"], r["source_on_interfaces"], r["source_levels"], mutation)
                + HO.midpoint_coefficients(r["dest_a"], r["dest_b"], r["dest_on_interfaces"], r["dest_levels"], mutation))
        mutation = None
    else:
        coef = midpoints(name)
    fields = {v: torch.from_numpy(inp[v]) for v in variables(name)}
    return {v: o.numpy() for v, o in HO.interp(fields, torch.from_numpy(inp["sp"]), *coef, dtype=dtype, mutation=mutation).items()}


@pytest.mark.parametrize("name", list(HYBRID_CASES))
def test_oracle_vs_reference_goldens(name):
    g, f32, f64, d_ref = load_golden(name, GOLD)
    inp = case_inputs(name, check=g)
    o32, o64 = run_oracle(name, inp, torch.float32), run_oracle(name, inp, torch.float64)
    bad = []
    for v in variables(name):
        assert o32[v].shape == f32[v].shape and o32[v].dtype == np.float32 and o64[v].dtype == np.float64, (name, v)
        d32 = distance(o32[v], f32[v])
        stored = np.abs(f64[v] - f32[v].astype(np.float64)) * 2.0 ** -24          # the rounding of the stored float32 difference
        over64 = float((np.abs(o64[v] - f64[v]) - stored).max() / np.abs(f64[v]).max())
        print(f"[hybrid oracle] {name} {v}: d_ref {d_ref[v]:.2e}; fp32 vs fp32 golden {d32:.2e} (<= 1e-6), fp64 vs fp64 golden beyond "
              f"the stored rounding {over64:.2e} (<= 1e-12)")
        if not (d32 <= 1e-6 and over64 <= 1e-12):
            bad.append((v, d32, over64))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", list(HYBRID_CASES))
def test_the_cases_meet_their_conditions(name):
    print(f"[hybrid cases] {name}: " + check_conditions(name, case_inputs(name)))
    sa, _, da, _ = midpoints(name)
    assert 2 <= sa.size <= 137 and 1 <= da.size <= 137


def test_the_level_index_variable_shows_bracket_and_weight():
    """`idx` comes back as lo + w: within [0, Ls - 1], and exactly 0 / Ls - 1 where the destination lies outside the source range."""
    _, f32, _, _ = load_golden("L13s2t", GOLD)
    y = f32["idx"]
    assert y.min() == 0.0 and y.max() == 12.0 and ((y > 0) & (y < 12)).any()


def test_the_goldens_catch_every_mutation():
    """Each broken rule moves some variable of some case beyond the gate against the fp64 golden (or makes it non-finite)."""
    caught = {m: [] for m in HO.MUTATIONS + HO.COEFFICIENT_MUTATIONS}
    for name in HYBRID_CASES:
        _, _, f64, d_ref = load_golden(name, GOLD)
        inp = case_inputs(name)
        for m in caught:
            try:
                out = run_oracle(name, inp, torch.float64, mutation=m)
                hit = any(out[v].shape != f64[v].shape or not np.isfinite(out[v]).all() or distance(out[v], f64[v]) > gate(d_ref[v])[1]
                          for v in variables(name))
            except (RuntimeError, IndexError):
                hit = True
            if hit:
                caught[m].append(name)
    for m, names in caught.items():
        print(f"[hybrid mutations] {m}: caught by {', '.join(names) or 'NO CASE'}")
    assert all(caught.values()), {m: n for m, n in caught.items() if not n}
