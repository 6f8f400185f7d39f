"""recon_amd.translation_residuals without a GPU: it is exported, and CPU tensors raise as everywhere in the package."""
import pytest
import torch


def test_translation_residuals_is_exported():
    import recon_amd
    from recon_amd.translation import translation_residuals
    assert recon_amd.translation_residuals is translation_residuals


def test_translation_residuals_rejects_cpu_tensors():
    from recon_amd import translation_residuals
    head, tail, W, rel = torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(3, 8, 8), torch.zeros(3, 8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        translation_residuals(head, tail, W, rel)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        translation_residuals(head[:0], tail[:0], W, rel)
