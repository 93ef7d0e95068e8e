"""CPU: the oracle against the reference for meshes of 4 to 8 coordinates, bit for bit.  tools/make_space_dim_golden.py ran
the reference's pit.py on these inputs: a masked cross layer (forward, attention matrix, d(values), d(lmda); periodic2d at
d = 4, per-sample meshes at d = 5) and a small pit_fixed with space_dim = d (forward and every parameter gradient)."""
import os

import numpy as np
import pytest
import torch

import pit_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


@pytest.mark.parametrize("d", [4, 5, 7, 8])
def test_layer_matches_reference_bitwise(d):
    z = _load(f"SD{d}_layer.npz")
    metric, batched, loc = str(z["metric"]), bool(z["batched"]), float(z["locality"])
    mesh_out, mesh_in = torch.from_numpy(z["mesh_out"]), torch.from_numpy(z["mesh_in"])
    assert mesh_in.shape[-1] == d
    lmda = torch.from_numpy(z["lmda"]).requires_grad_(True)
    values = torch.from_numpy(z["values"]).requires_grad_(True)
    out = orc.posatt_cross(metric, batched, mesh_out, mesh_in, values, lmda, loc)
    out.backward(torch.from_numpy(z["d_out"]))
    att = orc.attention_weights(orc.sqdist(metric, mesh_out, mesh_in), orc.head_scale(lmda.detach()), loc, batched)
    assert torch.equal(out.detach(), torch.from_numpy(z["out"]))
    assert torch.equal(att, torch.from_numpy(z["att"]))
    assert torch.equal(values.grad, torch.from_numpy(z["d_values"]))
    assert torch.equal(lmda.grad, torch.from_numpy(z["d_lmda"]))


@pytest.mark.parametrize("d", [4, 5, 7, 8])
def test_model_matches_reference_bitwise(d):
    z = _load(f"SD{d}_model.npz")
    p = {k[len("param:"):]: torch.from_numpy(z[k]).clone().requires_grad_(True) for k in z.files if k.startswith("param:")}
    assert p["en_layer.mlp1.weight"].shape[1] == 2 * (1 + d)          # n_head * (in_dim + space_dim), pit.py:100
    mesh_in, mesh_ltt = torch.from_numpy(z["mesh_in"]), torch.from_numpy(z["mesh_ltt"])
    loc = float(z["locality"])
    out = orc.pit_apply(p, "euclid", False, int(z["n_blocks"]), loc, loc, mesh_in, torch.from_numpy(z["func_in"]), mesh_ltt,
                        mesh_in)
    out.backward(torch.from_numpy(z["d_out"]))
    assert torch.equal(out.detach(), torch.from_numpy(z["out"]))
    for k in z.files:
        if k.startswith("grad:"):
            assert torch.equal(p[k[len("grad:"):]].grad, torch.from_numpy(z[k])), k
