"""Host side of kNN graphs wider than the shipped knn = 32: the model accepts 1 <= knn <= 64 (DD_KNN_MAX), nothing more."""
import os
import re

import pytest

from decompdiff_amd import DecompScorePosNet3D, shipped_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("knn", [1, 33, 48, 64])
def test_model_accepts_knn_up_to_64(knn):
    m = DecompScorePosNet3D(shipped_config(knn=knn), 29, 10, 8)
    assert m.config.knn == knn


@pytest.mark.parametrize("knn", [0, 65, 128])
def test_model_rejects_knn_outside_1_to_64(knn):
    with pytest.raises(NotImplementedError):
        DecompScorePosNet3D(shipped_config(knn=knn), 29, 10, 8)


def test_header_knn_max_is_64():
    with open(os.path.join(ROOT, "include", "decompdiff_hip.h")) as f:
        m = re.search(r"^#define DD_KNN_MAX (\d+)", f.read(), re.M)
    assert m and int(m.group(1)) == 64
