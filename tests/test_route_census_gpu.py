"""The complete set of launches of one forward, per configuration and switch set, against tests/golden/route_census.json.

test_variants_gpu / test_teacher_forced_gpu assert that certain kernels APPEAR on a route; this asserts the whole census -- every
profile row ("class.sSTAGE@family") with its launch count and the route counters of wx_query -- exactly.  The cases
(tools/make_route_census.CASES) are the smallest configurations at which each branch of the (attention, FeedForward) pair plan is
taken.  A route change made on purpose regenerates the fixture with tools/make_route_census.py; anything else that moves a row is a
dispatch bug."""
import json

import pytest

import make_route_census as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    with open(RC.FIXTURE) as f:
        return json.load(f)


def test_fixture_has_exactly_the_cases(fixture):
    assert sorted(fixture) == sorted(c["id"] for c in RC.CASES)


@pytest.mark.parametrize("case", RC.CASES, ids=[c["id"] for c in RC.CASES])
def test_route_census_equals_fixture(case, fixture):
    got, want = RC.census(case), fixture[case["id"]]
    rows = sorted(set(got["kernels"]) | set(want["kernels"]))
    diff = {r: (got["kernels"].get(r, 0), want["kernels"].get(r, 0)) for r in rows if got["kernels"].get(r, 0) != want["kernels"].get(r, 0)}
    assert not diff, f"{case['id']}: launches (got, fixture) differ on {diff}"
    assert got["queries"] == want["queries"], case["id"]
