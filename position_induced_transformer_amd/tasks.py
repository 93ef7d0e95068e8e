"""Task models: the ``forward`` wrappers the reference defines inside each train_*.py
(SURVEY section 8(f)-1), with the scripts' hyper-parameters as named constructors and
synthetic-data generators of the right shapes (the datasets are not in the reference
repository: supplementary_data/*.mat are LFS stubs).

All wrappers only reshape / concatenate and call encoder -> processor -> decoder of
:mod:`position_induced_transformer_amd.pit`; the arithmetic is in the HIP kernels.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import ops
from . import pit as P


# ----------------------------------------------------------------------------- meshes
def grid_mesh_2d(s: int, endpoint: bool = True, device=None) -> torch.Tensor:
    """(s, s, 2) grid in the point order of train_darcy.py:83-88 (endpoint) /
    train_vorticity.py:77-83 (periodic, linspace(0,1,s+1)[:-1])."""
    ax = np.linspace(0, 1, s) if endpoint else np.linspace(0, 1, s + 1)[:-1]
    m = np.vstack([xx.ravel() for xx in np.meshgrid(ax, ax)]).T.reshape(s, s, 2)
    return torch.tensor(m, dtype=torch.float, device=device)


def line_mesh_1d(n: int, lo: float = 0.0, hi: float = 1.0, device=None) -> torch.Tensor:
    """(n, 1) mesh linspace(lo,hi,n+1)[:-1] (train_burgers.py:59-60, train_sod.py:61-62)."""
    return torch.linspace(lo, hi, n + 1)[:-1].reshape(-1, 1).to(device)


# ----------------------------------------------------------------------------- wrappers
class _FixedMeshForward:
    """forward(mesh_in, func_in, mesh_out) of the fixed-mesh tasks: flatten, prepend the
    coordinates to the input function, encoder -> processor -> decoder
    (train_darcy.py:46-59, train_burgers.py:38-49, train_sod.py:42-53)."""

    residual = False

    def forward(self, mesh_in, func_in, mesh_out):
        self._mesh_grad(mesh_in, mesh_out)          # (refuses what the mesh-gradient path does not cover, before any launch)
        size = mesh_out.shape[:-1]
        batch = func_in.shape[0]
        mesh_in = mesh_in.reshape(-1, self.space_dim)
        mesh_out = mesh_out.reshape(-1, self.space_dim)
        func = func_in.reshape(batch, -1, self.in_dim)
        if isinstance(self.down, P.posatt) and func.is_cuda:
            # the coordinate concat of train_darcy.py:51-55 is deferred: the encoder's candidate-list kernels read the
            # coordinate channels from mesh_in (ops.tag_coords); any other consumer materialises the concat
            feats = ops.tag_coords(func, mesh_in)
        else:
            feats = torch.cat((mesh_in.unsqueeze(0).expand(batch, -1, -1), func), -1)
        ltt = self.encoder(mesh_in, feats, self.mesh_ltt)
        ltt = self._between(ltt)
        ltt = self.processor(ltt, self.mesh_ltt)
        ltt = self._between(ltt)
        out = self.decoder(self.mesh_ltt, ltt, mesh_out).reshape(batch, *size, self.out_dim)
        if self.residual:
            out = out + func_in.reshape(out.shape)
        return out

    def _between(self, x):
        return x


class pit_darcy(_FixedMeshForward, P.pit_fixed):
    """train_darcy.py:25-59."""


class pit_sod(_FixedMeshForward, P.pit_fixed):
    """train_sod.py:23-53."""


class pit_burgers(_FixedMeshForward, P.pit_periodic1d):
    """train_burgers.py:19-49."""


class pit_cylinder(_FixedMeshForward, P.pit_fixed):
    """train_cylinder.py:18-52: adds the input back onto the prediction."""
    residual = True


class pit_vorticity(_FixedMeshForward, P.pit_periodic2d):
    """train_vorticity.py:23-62: InstanceNorm1d over the points after encoder and processor."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.norm = nn.InstanceNorm1d(self.hid_dim)

    def _between(self, x):
        n = self.norm
        if x.is_cuda and isinstance(n, nn.InstanceNorm1d) and not n.affine and not n.track_running_stats:
            return ops.instance_norm_points(x, n.eps)          # HIP kernel on the (b, L, C) layout, no permutes
        return n(x.permute(0, 2, 1)).permute(0, 2, 1)


class pit_elasticity(P.pit):
    """train_elasticity.py:18-54: per-sample point cloud, latent mesh = output mesh."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.en_layer = P.kaiming_mlp(self.n_head * self.in_dim, self.hid_dim, self.hid_dim)

    def forward(self, mesh_in, func_in, mesh_out, len_in=None, len_out=None):
        """``len_in`` / ``len_out``: point counts of a ragged batch (padded clouds); the latent mesh is ``mesh_out``, so
        ``len_out`` is its length vector too, and ``len_in`` alone means both.  Padded rows of the result are finite
        (the decoder MLP's bias path) and meaningless: mask them, e.g. with ``RelLpNorm(...)(true, pred, lengths)``."""
        if len_in is not None or len_out is not None:
            len_in = len_out if len_in is None else len_in
            len_out = len_in if len_out is None else len_out
            size = mesh_out.shape[:-1]
            ltt = self.encoder(mesh_in, func_in, mesh_out, len_in=len_in, len_ltt=len_out)
            ltt = self.processor(ltt, mesh_out, len_ltt=len_out)
            return self.decoder(mesh_out, ltt, mesh_out, len_ltt=len_out, len_out=len_out).reshape(*size, self.out_dim)
        self._mesh_grad(mesh_in, mesh_out)
        size = mesh_out.shape[:-1]
        mesh_ltt = mesh_out
        ltt = self.encoder(mesh_in, func_in, mesh_ltt)
        ltt = self.processor(ltt, mesh_ltt)
        return self.decoder(mesh_ltt, ltt, mesh_out).reshape(*size, self.out_dim)


class pit_cloud_latent(P.pit):
    """Per-sample clouds on ONE latent mesh shared by the whole batch: the encoder projects every cloud onto the fixed
    ``mesh_ltt`` (L, space_dim) given to the constructor, the processor runs on it - the batch-free processor, no padding - and
    the decoder projects back onto each sample's own query points.  ``func_in`` is fed to the encoder as it is (``in_dim``
    channels, coordinates included if wanted, as in train_elasticity.py:39)."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        if self.mesh_ltt is None:
            raise ValueError("pit_cloud_latent needs the shared latent mesh (mesh_ltt)")
        self.mesh_ltt = self.mesh_ltt.contiguous()
        self.en_layer = P.kaiming_mlp(self.n_head * self.in_dim, self.hid_dim, self.hid_dim)

    def forward(self, mesh_in, func_in, mesh_out, len_in=None, len_out=None):
        """``mesh_in`` (b, n_in, space_dim) / ``mesh_out`` (b, n_out, space_dim): the clouds and the query points, padded;
        ``len_in`` / ``len_out``: their point counts (None = full width; ``len_in`` alone serves both when ``mesh_out`` IS
        ``mesh_in``).  The latent mesh has no length.  Padded rows of the result are finite (the decoder MLP's bias path)
        and meaningless: mask them, e.g. with ``RelLpNorm(...)(true, pred, lengths)``."""
        if ops.mesh_grad_wanted(self.mesh_ltt, mesh_in, mesh_out):         # (before anything is launched)
            raise NotImplementedError("a mesh that requires grad in a mixed pair: mesh gradients are not implemented for a shared "
                                      "mesh against per-sample clouds")
        if len_out is None and len_in is not None and mesh_out is mesh_in:
            len_out = len_in
        size = mesh_out.shape[:-1]
        mesh_ltt = self.mesh_ltt if self.mesh_ltt.device == mesh_in.device else self.mesh_ltt.to(mesh_in.device)
        self.mesh_ltt = mesh_ltt
        ltt = self.encoder(mesh_in, func_in, mesh_ltt, len_in=len_in)
        ltt = self.processor(ltt, mesh_ltt)
        return self.decoder(mesh_ltt, ltt, mesh_out, len_out=len_out).reshape(*size, self.out_dim)


class pit_cloud_fps(P.pit):
    """Per-sample clouds on a latent mesh chosen per cloud FROM the cloud: ``n_latent`` points by farthest-point sampling
    (ops.farthest_point_sample - one launch inside the step, so a captured step samples the clouds it is fed; clouds beyond that
    sampler's envelope go through ops.farthest_point_sample_large, one launch per latent point, with the same picks).  What
    ``pit_naca.ltt_mesh`` does with strides on a structured grid, for clouds that have no structure to stride over: the
    processor's dense self-attention runs on n_latent x n_latent instead of n x n per sample.  ``func_in`` is fed to the
    encoder as it is (``in_dim`` channels, coordinates included if wanted, as in train_elasticity.py:39)."""

    def __init__(self, space_dim, in_dim, out_dim, hid_dim, n_head, n_blocks, n_latent, en_loc, de_loc, start=0):
        super().__init__(space_dim, in_dim, out_dim, hid_dim, n_head, n_blocks, None, en_loc, de_loc)
        if isinstance(n_latent, bool) or not isinstance(n_latent, (int, np.integer)) or n_latent < 1:
            raise ValueError(f"n_latent must be a positive integer, got {n_latent!r}")
        self.n_latent = int(n_latent)
        self.start = start
        self.last_latent = None
        self.en_layer = P.kaiming_mlp(self.n_head * self.in_dim, self.hid_dim, self.hid_dim)

    def forward(self, mesh_in, func_in, mesh_out, len_in=None, len_out=None):
        """``mesh_in`` (b, n_in, space_dim) / ``mesh_out`` (b, n_out, space_dim): the clouds and the query points, padded;
        ``len_in`` / ``len_out``: their point counts (None = full width; ``len_in`` alone serves both when ``mesh_out`` IS
        ``mesh_in``).  The latent mesh is the sampling of ``mesh_in`` under ``len_in``: a cloud shorter than ``n_latent`` has
        as many latent points as it has points.  Without lengths the plain per-sample path runs (any math mode; then
        ``n_latent <= n_in``), and a mesh that requires grad receives its gradient through the chosen points (the choice
        itself is a constant).  ``last_latent``: the ``ops.FpsResult`` of this call.  Padded rows of the result are finite
        and meaningless: mask them, e.g. with ``RelLpNorm(...)(true, pred, lengths)``."""
        if not torch.is_tensor(mesh_in) or mesh_in.dim() != 3:
            raise ValueError("pit_cloud_fps needs per-sample (batch, n, space_dim) clouds")
        if len_out is None and len_in is not None and mesh_out is mesh_in:
            len_out = len_in
        ragged = len_in is not None or len_out is not None
        if ragged:
            if len_in is None or len_out is None:
                raise ValueError("pit_cloud_fps: a ragged batch needs len_in (and len_out, unless mesh_out is mesh_in)")
            ops.check_ragged("euclid", mesh_out, mesh_in)              # (before anything is launched)
            len_in = ops.as_lengths(len_in, mesh_in.device, mesh_in.shape[0])
        else:
            self._mesh_grad(mesh_in, mesh_out)
        if mesh_in.shape[1] <= ops.fps_max_points(mesh_in.shape[2]):
            latent = ops.farthest_point_sample(mesh_in, self.n_latent, len_in, self.start)
        else:                                                          # (the same picks, one launch per pick)
            latent = ops.farthest_point_sample_large(mesh_in, self.n_latent, len_in, self.start)
        self.last_latent = latent
        size = mesh_out.shape[:-1]
        if ragged:
            ltt, len_ltt = latent.mesh, latent.lengths
            f = self.encoder(mesh_in, func_in, ltt, len_in=len_in, len_ltt=len_ltt)
            f = self.processor(f, ltt, len_ltt=len_ltt)
            return self.decoder(ltt, f, mesh_out, len_ltt=len_ltt, len_out=len_out).reshape(*size, self.out_dim)
        ltt = latent.mesh
        if torch.is_grad_enabled() and mesh_in.requires_grad:
            # the same bits as latent.mesh, as a differentiable function of mesh_in
            ltt = torch.gather(mesh_in, 1, latent.idx.long().unsqueeze(-1).expand(-1, -1, mesh_in.shape[-1]))
        f = self.encoder(mesh_in, func_in, ltt)
        f = self.processor(f, ltt)
        return self.decoder(ltt, f, mesh_out).reshape(*size, self.out_dim)


class pit_naca(P.pit):
    """train_naca.py:17-65: latent mesh = strided sub-grid of the body-fitted output grid."""

    def __init__(self, space_dim, in_dim, out_dim, hid_dim, n_head, n_blocks, mesh_ltt, x_downsample,
                 y_downsample, en_loc, de_loc):
        super().__init__(space_dim, in_dim, out_dim, hid_dim, n_head, n_blocks, mesh_ltt, en_loc, de_loc)
        self.x_down, self.y_down = x_downsample, y_downsample
        self.x_res = int(220 / x_downsample) + 1
        self.y_res = int(50 / y_downsample) + 1
        self.en_layer = P.kaiming_mlp(self.n_head * self.in_dim, self.hid_dim, self.hid_dim)

    def ltt_mesh(self, mesh_out):
        b = mesh_out.shape[0]
        ltt = mesh_out[:, ::self.x_down, ::self.y_down, :][:, :self.x_res, :self.y_res, :]
        return ltt.reshape(b, -1, self.space_dim), mesh_out.reshape(b, -1, self.space_dim)

    def forward(self, mesh_in, func_in, mesh_out):
        self._mesh_grad(mesh_in, mesh_out)
        size = mesh_out.shape[:-1]
        mesh_ltt, mesh_flat = self.ltt_mesh(mesh_out)
        ltt = self.encoder(mesh_in, func_in, mesh_ltt)
        ltt = self.processor(ltt, mesh_ltt)
        return self.decoder(mesh_ltt, ltt, mesh_flat).reshape(*size, self.out_dim)


class _RecomputedStep(torch.autograd.Function):
    """One rollout step whose forward keeps ONLY its input: the prediction is computed under no_grad, and the backward
    re-runs the step's forward with autograd on and back-propagates through it (parameter gradients accumulate into
    ``.grad`` as in any backward pass, the input gradient is returned).  Nothing but kernel launches on the current
    stream, so - unlike torch.utils.checkpoint with its saved-tensor hooks and RNG bookkeeping - the whole rollout
    stays capturable into one hipGraph (engine.RolloutStep(recompute=True)).  ``anchor`` is a scalar that requires
    grad: the first step's input is data, and a node none of whose inputs requires grad would never be visited."""

    @staticmethod
    def forward(ctx, anchor, model, mesh, x):
        ctx.model, ctx.mesh = model, mesh
        ctx.save_for_backward(x)
        with torch.no_grad():
            return model(mesh, x, mesh)

    @staticmethod
    def backward(ctx, d_out):
        (x,) = ctx.saved_tensors
        xd = x.detach().requires_grad_(True)
        with torch.enable_grad():
            out = ctx.model(ctx.mesh, xd, ctx.mesh)
        torch.autograd.backward(out, d_out)
        return None, None, None, xd.grad


def rollout_loss(model, mesh, x, y, steps: int, loss_fn, recompute: bool = False):
    """Autoregressive training objective of train_vorticity.py:118-126: ``steps`` successive
    predictions, each appended to the input history (oldest frame dropped), loss summed over the
    steps with the arguments in the script's order ``loss_fn(out, y_t)``; back-propagates through
    the whole rollout.

    Memory: one forward of the full configuration (64x64 grid, hid 256, batch 20) saves ~0.49 GB for its
    backward (decoder attention output and decoder-MLP pre-activations dominate), so the 20-step rollout
    holds ~10 GB - 3.5 % of the MI355X's 288 GB: nothing has to be recomputed, which is the default.
    ``recompute=True`` keeps only each step's input and re-runs that step's forward inside the backward
    pass (_RecomputedStep: +1 forward per step, ~25x less activation memory, capturable) for rollouts /
    batches that would not fit."""
    loss = 0.0
    anchor = torch.ones((), device=x.device, requires_grad=True) if recompute else None
    for t in range(steps):
        if recompute:
            out = _RecomputedStep.apply(anchor, model, mesh, x)
        else:
            out = model(mesh, x, mesh)
        loss = loss + loss_fn(out, y[..., t:t + 1])
        x = torch.cat((x[..., 1:], out), dim=-1)
    return loss


# ----------------------------------------------------------------------------- configs
def ragged_clouds(lengths, width: int, space_dim: int = 2, channels: int = 1, out_dim: int = 1, device="cpu", seed: int = 0,
                  pad_value: float = 0.0):
    """Synthetic ragged batch of point clouds for tests and examples: sample s has lengths[s] points uniform in the unit
    cube, an input function and a target, each padded to ``width`` points with ``pad_value`` (NaN shows that padding
    never enters the arithmetic).  Returns (mesh, func, target, lengths as an int32 tensor), all on ``device``."""
    g = torch.Generator().manual_seed(seed)
    b = len(lengths)
    mesh = torch.full((b, width, space_dim), pad_value)
    func = torch.full((b, width, channels), pad_value)
    target = torch.full((b, width, out_dim), pad_value)
    for s, n in enumerate(lengths):
        if not 1 <= n <= width:
            raise ValueError(f"length {n} outside [1, {width}]")
        mesh[s, :n] = torch.rand((n, space_dim), generator=g)
        func[s, :n] = torch.randn((n, channels), generator=g)
        target[s, :n] = torch.randn((n, out_dim), generator=g)
    return mesh.to(device), func.to(device), target.to(device), torch.tensor(list(lengths), dtype=torch.int32, device=device)


def make_task(name: str, device="cuda", seed: int = 0):
    """Build (model, sample_fn) for a named configuration of the reference.

    ``sample_fn(batch, seed)`` returns ``(mesh_in, func_in, mesh_out, target)`` synthetic
    tensors on ``device`` with the shapes the corresponding train script feeds."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)

    def randn(*shape):
        return torch.randn(*shape, generator=g).to(device)

    def rand(*shape):
        return torch.rand(*shape, generator=g).to(device)

    if name == "darcy":                     # train_darcy.py:64-111
        mesh, ltt = grid_mesh_2d(43, True, device), grid_mesh_2d(16, True, device)
        model = pit_darcy(2, 1, 1, 64, 2, 4, ltt, 0.02, 0.02)
        sample = lambda b: (mesh, randn(b, 43, 43, 1), mesh, randn(b, 43, 43, 1))  # noqa: E731
        meta = dict(out_dim=1, p=2, batch=8)
    elif name == "burgers":                 # train_burgers.py:51-72
        mesh, ltt = line_mesh_1d(1024, device=device), line_mesh_1d(256, device=device)
        model = pit_burgers(1, 1, 1, 64, 2, 5, ltt, 0.02, 0.02)
        sample = lambda b: (mesh, randn(b, 1024, 1), mesh, randn(b, 1024, 1))  # noqa: E731
        meta = dict(out_dim=1, p=1, batch=8)
    elif name == "sod":                     # train_sod.py:55-76 (N = 1024 points on [-5,5))
        mesh, ltt = line_mesh_1d(1024, -5, 5, device), line_mesh_1d(256, -5, 5, device)
        model = pit_sod(1, 3, 3, 32, 1, 2, ltt, 0.02, 0.02)
        sample = lambda b: (mesh, randn(b, 1024, 3), mesh, randn(b, 1024, 3))  # noqa: E731
        meta = dict(out_dim=3, p=1, batch=8)
    elif name == "vorticity":               # train_vorticity.py:65-106
        mesh, ltt = grid_mesh_2d(64, False, device), grid_mesh_2d(16, False, device)
        model = pit_vorticity(2, 10, 1, 256, 2, 4, ltt, 0.02, 0.02)
        sample = lambda b: (mesh, randn(b, 64, 64, 10), mesh, randn(b, 64, 64, 1))  # noqa: E731
        meta = dict(out_dim=1, p=2, batch=20)
    elif name == "elasticity":              # train_elasticity.py:56-75, 972-point clouds
        model = pit_elasticity(2, 44, 1, 256, 2, 4, None, 0.02, 0.02)

        def sample(b):
            xy = rand(b, 972, 2)
            feats = torch.cat((xy, rand(b, 972, 42) * 5 - 1), -1)      # 5*R-1 of train_elasticity.py:12
            return xy, feats, xy, randn(b, 972, 1)
        meta = dict(out_dim=1, p=2, batch=10)
    elif name == "naca":                    # train_naca.py:68-89: 120 -> 728 -> 221x51
        model = pit_naca(2, 2, 4, 128, 1, 4, None, 4, 4, 0.02, 0.02)

        def sample(b):
            th = torch.linspace(0, 2 * np.pi, 121)[:-1]
            ax = 0.5 + 0.1 * torch.rand(b, 1, generator=g)
            by = 0.06 + 0.03 * torch.rand(b, 1, generator=g)
            outline = torch.stack((ax * torch.cos(th), by * torch.sin(th)), -1)            # (b,120,2)
            t221 = torch.linspace(0, 2 * np.pi, 222)[:-1]
            r = torch.linspace(0, 1, 51) ** 1.5 * 4.0                                      # O-grid radii
            gx = (ax.unsqueeze(-1) + r) * torch.cos(t221).reshape(1, -1, 1)
            gy = (by.unsqueeze(-1) + r) * torch.sin(t221).reshape(1, -1, 1)
            grid = torch.stack((gx, gy), -1) + 1e-3 * torch.randn(b, 221, 51, 2, generator=g)
            return outline.to(device), outline.to(device), grid.to(device), randn(b, 221, 51, 4)
        meta = dict(out_dim=4, p=2, batch=20)
    elif name == "cylinder":                # train_cylinder.py:55-84: 4390 -> 896 -> 4390 (unstructured)
        mesh = torch.rand(4390, 2, generator=g).to(device) * torch.tensor([4.0, 2.0], device=device)
        ltt = mesh[torch.randperm(4390, generator=g)[:896].to(device)].contiguous()
        model = pit_cylinder(2, 3, 3, 256, 1, 4, ltt, 0.01, 0.01)
        sample = lambda b: (mesh, randn(b, 4390, 3), mesh, randn(b, 4390, 3))  # noqa: E731
        meta = dict(out_dim=3, p=2, batch=200)
    else:
        raise KeyError(name)
    return model.to(device), sample, meta


TASKS = ("darcy", "burgers", "sod", "vorticity", "elasticity", "naca", "cylinder")
