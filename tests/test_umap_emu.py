"""UMAP (vame_amd/csrc/umap.hip + vame_amd/analysis/umap_hip.py + vame.visualization) through the host emulator, small shapes;
the same cases run on the MI355X in test_umap_gpu.py."""
import pytest

from umap_cases import (check_epoch, check_graph, check_knn, check_knn_duplicates, check_knn_errors, check_membership, check_pipeline,
                        check_visualization)

DEV = "cpu"


@pytest.mark.parametrize("N,D,k", [(300, 30, 15), (500, 5, 200), (257, 64, 2)])
def test_knn(emu, N, D, k):
    check_knn(DEV, N, D, k)


def test_knn_duplicate_points_keep_the_tie_rule(emu):
    check_knn_duplicates(DEV)


def test_knn_argument_checks(emu):
    check_knn_errors(DEV)


def test_membership(emu):
    check_membership(DEV)


def test_fuzzy_union_graph(emu):
    check_graph(DEV)


def test_layout_epoch(emu):
    check_epoch(DEV)


def test_pipeline(emu):
    check_pipeline(DEV)


def test_visualization(emu, tmp_path, monkeypatch):
    check_visualization(tmp_path, monkeypatch)
