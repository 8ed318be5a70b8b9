"""The wide tier behind the paged and the depth calls of the subjects handle
(ketogpu_subjects_page_wide / ketogpu_subjects_ids_depth_wide): wide_page_gpu_suite.py's checks over
the forward rows."""
import pytest

from tests import lookup_cases as LC
from tests import wide_gpu_suite as W
from tests import wide_page_gpu_suite as P

pytestmark = pytest.mark.gpu
S = P.SUBJECTS


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    W.need_gpu()


@pytest.fixture(params=[False, True], ids=["default", "forced"])
def forced(request):
    return request.param


@pytest.mark.parametrize("case", LC.TABLES, ids=lambda c: f"seed{c[0]}")
def test_truth_tables(case, forced, monkeypatch):
    P.check_truth_table(S, case, forced, monkeypatch)


def test_a_limit_of_k_hops_is_k_level_launches(monkeypatch):
    P.check_chain_levels(S, monkeypatch)


def test_structure_cases(monkeypatch):
    P.check_structure_cases(S, monkeypatch)


def test_one_round_with_different_limits(monkeypatch):
    P.check_mixed_round(S, monkeypatch)


@pytest.mark.parametrize("slots", [1, 2])
def test_rounds_and_one_start_twice(slots, monkeypatch):
    P.check_rounds(S, slots, monkeypatch)


def test_finish_boundaries_of_a_large_list():
    P.check_boundaries_big(S)


def test_finish_boundaries_of_a_sparse_list(monkeypatch):
    P.check_boundaries_sparse(S, monkeypatch)


def test_every_finish_leaves_the_bitmaps_zero(monkeypatch):
    P.check_bitmaps_left_zero(S, monkeypatch)


def test_contracts(forced, monkeypatch):
    P.check_contracts(S, forced, monkeypatch)


def test_writes_are_seen_by_the_next_wide_page(monkeypatch):
    P.check_writes(S, monkeypatch)
