"""CPU: the order in which the kernels add squared coordinate differences for meshes of 4 to 8 coordinates (pit_common.h
sq_dist8t) reproduces torch.sum over the last axis - the reference's distance (pit.py:47,134,253) - bit
for bit, and the library accepts exactly space_dim 1..8."""
import pytest
import torch


def kernel_order_sum(q: torch.Tensor) -> torch.Tensor:
    """sq_dist8t's order on fp32 terms q (..., d), d <= 8: left to right for d <= 4 and d = 8; for d = 5, 6, 7
    ((((q0 + q4) + q5) + q6) + q1) + q2) + q3 with the missing terms left out."""
    d = q.shape[-1]
    t = [q[..., k] for k in range(d)]
    if 5 <= d <= 7:
        s = t[0] + t[4]
        for k in range(5, d):
            s = s + t[k]
        for k in (1, 2, 3):
            s = s + t[k]
        return s
    s = t[0]
    for k in range(1, d):
        s = s + t[k]
    return s


@pytest.mark.parametrize("d", range(1, 9))
def test_kernel_order_reproduces_torch_sum(d):
    g = torch.Generator().manual_seed(d)
    a = torch.rand(300, 1, d, generator=g)
    b = torch.rand(1, 400, d, generator=g)
    q = (a - b) ** 2
    assert torch.equal(kernel_order_sum(q), torch.sum(q, -1))


@pytest.mark.parametrize("d", [4, 5, 6, 7, 8])
def test_kernel_order_on_lattices_and_periodic_terms(d):
    """Tie-heavy lattices and the periodic wrap min(|x|, l - |x|) of pit.py:251-253 go through the same order."""
    axes = [torch.linspace(0.0, 1.0, 3)] * d
    mesh = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, d)
    diff = (mesh[:, None, :] - mesh[None, :, :]).abs()
    l = torch.tensor(1.5)
    for m in (diff, torch.minimum(diff, l - diff)):
        q = m ** 2
        assert torch.equal(kernel_order_sum(q), torch.sum(q, -1))


def test_order_differs_from_left_to_right_for_5_to_7():
    """The case the kernels must not get wrong: a plain left-to-right sum disagrees with torch.sum for d = 5, 6, 7."""
    g = torch.Generator().manual_seed(0)
    for d in (5, 6, 7):
        q = torch.rand(20000, d, generator=g) ** 2
        seq = q[:, 0]
        for k in range(1, d):
            seq = seq + q[:, k]
        assert not torch.equal(seq, torch.sum(q, -1))


def test_library_limit_is_eight():
    import os
    from position_induced_transformer_amd import ops
    assert ops.MAX_SPACE_DIM == 8
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pit_hip.h")).read()
    assert "#define PIT_MAX_SPACE_DIM 8 " in header


def test_fused_predicates_step_aside_beyond_three_coordinates():
    from position_induced_transformer_amd import ops
    assert not ops.block_fusion_supported(256, 2, 32, 4, space_dim=4)
    assert not ops.pre_weights_supported(4096, 2, 64, 4, space_dim=5)
