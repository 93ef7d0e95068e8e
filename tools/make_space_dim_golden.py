"""Generate tests/golden/SD{4,5,7,8}_*.npz: reference results for meshes of 4 to 8 coordinates.

Run:  python tools/make_space_dim_golden.py     (needs the reference's pit.py on the path given by PIT_REFERENCE; CPU only)

For every case the reference (its pit.py, imported unmodified) and the oracle (oracle/pit_oracle.py) run on the same seeded
inputs.  The script asserts that their results are bit-equal and stores inputs and expected outputs as plain arrays:
  * layer: a masked cross layer (per-sample meshes for d = 5, batch-free otherwise; periodic2d for d = 4) - the forward, the
    attention matrix, d(values) and d(lmda) for a fixed output gradient;
  * model: a small pit_fixed with space_dim = d (encoder width n_head * (in_dim + space_dim)) - the forward and the gradient
    of every parameter for a fixed output gradient.
tests/test_space_dim_golden.py holds the oracle to these files bit for bit.  No test runs this script.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.environ.get("PIT_REFERENCE", "/root/reference"))
import pit as ref            # noqa: E402  the reference, read-only
import pit_oracle as orc     # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(4)

LAYERS = {  # d: (metric, batched)
    4: ("periodic2d", False),
    5: ("euclid", True),
    7: ("euclid", False),
    8: ("euclid", False),
}
REF_CROSS = {("euclid", True): ref.posatt_cross, ("euclid", False): ref.posatt_cross_fixed,
             ("periodic2d", False): ref.posatt_cross_periodic2d}


def npf(t):
    return t.detach().cpu().numpy()


def lattice(n, d):
    axes = [torch.linspace(0.0, 1.0, n)] * d
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, d).contiguous()


def layer_case(d):
    metric, batched = LAYERS[d]
    g = torch.Generator().manual_seed(100 + d)
    b, n_head, dim, loc = 2, 2, 6, 0.1
    if metric == "periodic2d":
        mesh_in = lattice(3, d)                     # 81 points: a square grid along axis 0 (pit.py:248-250)
        mesh_out = mesh_in[::2].contiguous()
    else:
        mesh_in = torch.rand((b, 90, d) if batched else (90, d), generator=g)
        mesh_out = torch.rand((b, 50, d) if batched else (50, d), generator=g)
    values = torch.randn(b, mesh_in.shape[-2], dim, generator=g)
    lmda = torch.randn(n_head, 1, 1, generator=g) * 0.5
    gout = torch.randn(b, mesh_out.shape[-2], n_head * dim, generator=g)

    mod = REF_CROSS[(metric, batched)](n_head, dim, loc)
    with torch.no_grad():
        mod.lmda.copy_(lmda)
    v_ref = values.clone().requires_grad_(True)
    out_ref = mod(mesh_out, mesh_in, v_ref)
    out_ref.backward(gout)
    att_ref = mod.dist2att(mesh_out, mesh_in, mod.lmda, loc)

    lm = lmda.clone().requires_grad_(True)
    v_orc = values.clone().requires_grad_(True)
    out_orc = orc.posatt_cross(metric, batched, mesh_out, mesh_in, v_orc, lm, loc)
    out_orc.backward(gout)
    att_orc = orc.attention_weights(orc.sqdist(metric, mesh_out, mesh_in), orc.head_scale(lmda), loc, batched)

    assert torch.equal(out_ref, out_orc), f"d={d}: forward"
    assert torch.equal(att_ref, att_orc), f"d={d}: attention"
    assert torch.equal(v_ref.grad, v_orc.grad), f"d={d}: d(values)"
    assert torch.equal(mod.lmda.grad, lm.grad), f"d={d}: d(lmda)"
    np.savez_compressed(os.path.join(OUT, f"SD{d}_layer.npz"), metric=metric, batched=batched, locality=loc,
                        mesh_out=npf(mesh_out), mesh_in=npf(mesh_in), values=npf(values), lmda=npf(lmda), d_out=npf(gout),
                        out=npf(out_ref), att=npf(att_ref), d_values=npf(v_ref.grad), d_lmda=npf(mod.lmda.grad))


def model_case(d):
    g = torch.Generator().manual_seed(200 + d)
    torch.manual_seed(200 + d)
    b, in_dim, out_dim, hid, n_head, n_blocks, loc = 2, 1, 1, 8, 2, 1, 0.1
    mesh_in = torch.rand(60, d, generator=g)
    mesh_ltt = torch.rand(20, d, generator=g)
    func = torch.cat((mesh_in.unsqueeze(0).expand(b, -1, -1), torch.randn(b, 60, in_dim, generator=g)), -1)
    gout = torch.randn(b, 60, out_dim, generator=g)
    model = ref.pit_fixed(d, in_dim, out_dim, hid, n_head, n_blocks, mesh_ltt, loc, loc)
    out_ref = model.decoder(mesh_ltt, model.processor(model.encoder(mesh_in, func, mesh_ltt), mesh_ltt), mesh_in)
    out_ref.backward(gout)

    p = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    out_orc = orc.pit_apply(p, "euclid", False, n_blocks, loc, loc, mesh_in, func, mesh_ltt, mesh_in)
    out_orc.backward(gout)
    assert torch.equal(out_ref, out_orc), f"d={d}: model forward"
    grads = {}
    for name, prm in model.named_parameters():
        assert torch.equal(prm.grad, p[name].grad), f"d={d}: {name}"
        grads["grad:" + name] = npf(prm.grad)
    params = {"param:" + k: npf(v) for k, v in model.state_dict().items()}
    np.savez_compressed(os.path.join(OUT, f"SD{d}_model.npz"), n_blocks=n_blocks, locality=loc, mesh_in=npf(mesh_in),
                        mesh_ltt=npf(mesh_ltt), func_in=npf(func), d_out=npf(gout), out=npf(out_ref), **params, **grads)


if __name__ == "__main__":
    for d in (4, 5, 7, 8):
        layer_case(d)
        model_case(d)
        print("SD%d: reference == oracle, written" % d)
