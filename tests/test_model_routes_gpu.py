"""Every model class at the smallest shape that reaches each of its routes: the rungs layer_stack.run takes and the engine's
kernel names of one forward + backward, against the table recorded before layer_stack existed (tests/model_routes_cases.py;
tools/model_routes.py prints the same cases with grids and output bits)."""
import pytest

from tests import model_routes_cases as K
from tests.judging import dev  # noqa: F401

pytestmark = pytest.mark.gpu


def test_every_case_has_its_record():
    assert set(K.EXPECTED) == set(K.CASES)


@pytest.mark.parametrize("case", list(K.CASES))
def test_route(dev, case, monkeypatch):  # noqa: F811
    from pde_policylearning_amd import layer_stack as LS
    rungs_want, kernels_want = K.EXPECTED[case]
    rungs, route = [], LS.route
    monkeypatch.setattr(LS, "route", lambda *a: rungs.append(route(*a)) or rungs[-1])      # what run() is told, in call order
    if kernels_want == "refused":
        with pytest.raises(RuntimeError):
            K.run_case(case, K.CASES[case], dev)
    else:
        records, _ = K.run_case(case, K.CASES[case], dev)
        assert [r["name"] for r in records] == K.expand(kernels_want)
    assert rungs == rungs_want.split()
