"""UMAP on the MI355X: the emulator's kernel cases on `cuda`, the kNN at the stock shape, layout quality, determinism and
vame.visualization() at the stock configuration.  Run with -m gpu."""
import pytest

from umap_cases import (check_determinism, check_epoch, check_graph, check_knn, check_knn_duplicates, check_knn_errors, check_layout_blobs,
                        check_layout_curve, check_membership, check_pipeline, check_visualization, check_visualization_stock)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("N,D,k", [(300, 30, 15), (500, 5, 200), (257, 64, 2)])
def test_knn(hip, N, D, k):
    check_knn(DEV, N, D, k)


def test_knn_stock_shape(hip):
    """N = 30000, D = 30, k = 200 (the reference's num_points / n_neighbors defaults) against float64 on 2000 sampled rows"""
    check_knn(DEV, 30000, 30, 200, n_check=2000)


def test_knn_duplicate_points_keep_the_tie_rule(hip):
    check_knn_duplicates(DEV)


def test_knn_argument_checks(hip):
    check_knn_errors(DEV)


def test_membership(hip):
    check_membership(DEV)


def test_fuzzy_union_graph(hip):
    check_graph(DEV)


def test_layout_epoch(hip):
    check_epoch(DEV)


def test_pipeline(hip):
    check_pipeline(DEV)


def test_layout_separates_blobs(hip):
    check_layout_blobs(DEV)


def test_layout_keeps_a_closed_curve(hip):
    check_layout_curve(DEV)


def test_layout_is_bitwise_reproducible(hip):
    check_determinism(DEV)


def test_visualization(hip, tmp_path, monkeypatch):
    check_visualization(tmp_path, monkeypatch)


def test_visualization_stock_configuration(hip, tmp_path):
    check_visualization_stock(tmp_path)
