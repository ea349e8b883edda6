"""Fixtures that several GPU test modules share (imported by name where they are used; this is not a conftest)."""
import pytest


@pytest.fixture(params=["fused", "records"])
def build_path(request, monkeypatch):
    """Both normal-equation builds of the library: the fused build (k_build_visual, default wherever a landmark's window has <= 256 tiles)
    and the record path (HS_BUILD_PATH=records: k_linearize_visual -> k_landmark -> Gram kernels; what long feature tracks always take)."""
    monkeypatch.setenv("HS_BUILD_PATH", request.param)
    return request.param
