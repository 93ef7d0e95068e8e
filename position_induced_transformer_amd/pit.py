"""Drop-in replacement for the reference's ``pit.py`` (``from pit import *``).

Same class names, constructor signatures, attribute and parameter names and the same
star-exports (``torch, nn, gelu, np, pi``) as /root/reference/pit.py, so the
``train_*.py`` scripts run unchanged; the arithmetic of every operator is done by the
hand-written gfx950 kernels behind include/pit_hip.h (position_induced_transformer_amd.ops).

The reference module has import-time side effects that its scripts rely on (pit.py:2-10:
``torch.manual_seed(0)``, ``torch.cuda.manual_seed(0)``, ``np.random.seed(0)``, the cudnn flags
and ``set_float32_matmul_precision('high')``): a script that never seeds gets the SAME initial
weights on every run because ``from pit import *`` seeded for it.  They are reproduced here, at
import, so such a script initialises seed-for-seed like the reference; set
``PIT_IMPORT_SIDE_EFFECTS=0`` in the environment to import without touching global state.

``model = torch.compile(model)`` (train_darcy.py:112 and every other script) works unchanged:
the operators already are fused kernels, so a task subclass's ``forward`` is marked
``torch.compiler.disable`` when the class is created (``pit.__init_subclass__``) and dynamo runs
the module eagerly - no graph is traced, no Triton is generated, ``state_dict()`` of the wrapper
carries the ``_orig_mod.`` keys of train_darcy.py:150.  The four operator entry points in ``ops``
are opaque to dynamo as well, for code that compiles something other than a ``pit`` subclass.

Differences that are deliberate:
  * the (b,H,N,J) attention tensor is never materialised in ``forward``; ``dist2att`` /
    ``convolution`` remain as explicit dense helpers for API compatibility only;
  * mesh-dependent selection statistics are cached per (mesh, locality) for fixed meshes.
"""
from __future__ import annotations

import functools
import os
from collections import OrderedDict
from math import pi

import numpy as np
import torch
import torch.nn as nn
from torch.nn.functional import gelu

from . import ops

if os.environ.get("PIT_IMPORT_SIDE_EFFECTS", "1") != "0":      # pit.py:2-10, reproduced (see the docstring)
    torch.set_float32_matmul_precision("high")
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)          # lazy: harmless without a GPU
    torch.backends.cudnn.benchmark = True
    torch.backends.cudnn.deterministic = True
    np.random.seed(0)

__all__ = [
    "kaiming_mlp", "posatt", "posatt_cross", "pit",
    "posatt_fixed", "posatt_cross_fixed", "pit_fixed",
    "posatt_periodic1d", "posatt_cross_periodic1d", "pit_periodic1d",
    "posatt_periodic2d", "posatt_cross_periodic2d", "pit_periodic2d",
    "torch", "nn", "gelu", "np", "pi",
]


def _eager_under_dynamo(fwd):
    """``fwd`` behind a plain function whose body is one call into a ``torch.compiler.disable``d copy:
    dynamo finds nothing to trace.  The disable wrapper itself is not installed as ``forward`` because
    its ``_torchdynamo_orig_callable`` attribute (the UNBOUND function) would be unwrapped by
    ``torch._dynamo.disable(model)`` (train_darcy.py:152) and called without ``self``."""
    inner = torch.compiler.disable(fwd)

    @functools.wraps(fwd)
    def forward(self, *args, **kwargs):
        return inner(self, *args, **kwargs)
    forward._pit_eager = True
    return forward


class kaiming_mlp(nn.Module):
    """Linear -> exact-erf GELU -> Linear with He-normal weights (pit.py:13-26).
    Parameters: ``mlp1.weight, mlp1.bias, mlp2.weight, mlp2.bias``."""

    def __init__(self, n_filters0, n_filters1, n_filters2):
        super().__init__()
        self.mlp1 = nn.Linear(n_filters0, n_filters1)
        self.mlp2 = nn.Linear(n_filters1, n_filters2)
        nn.init.kaiming_normal_(self.mlp1.weight)
        nn.init.kaiming_normal_(self.mlp2.weight)

    def forward(self, x, out_gelu: bool = False, concat_heads: int = 0, ordered: bool = False):
        """``out_gelu=True`` fuses the gelu that pit.encoder/processor apply to the result
        (pit.py:111,121) into the second GEMM's epilogue; ``concat_heads=H`` writes the result into the
        concat buffer of the H-head self-attention layer that consumes it (ops.mlp_apply)."""
        return ops.mlp_apply(x, self.mlp1.weight, self.mlp1.bias, self.mlp2.weight, self.mlp2.bias, out_gelu,
                             concat_heads, ordered)


class posatt(nn.Module):
    """Position attention on per-sample meshes, self-attention form (pit.py:28-57).
    ``forward(mesh, inputs)`` returns ``cat((inputs, conv), -1)``."""

    _metric = "euclid"
    _batched = True
    _PLAN_CACHE = 8

    def __init__(self, n_head, in_dim, locality):
        super().__init__()
        self.locality = locality
        self.n_head = n_head
        self.in_dim = in_dim
        self.lmda = nn.Parameter(torch.rand(n_head, 1, 1))
        self._plans = OrderedDict()          # LRU of mesh plans (batch-free meshes)

    # -- selection statistics: cached for fixed meshes, rebuilt per call for per-sample meshes
    def _plan(self, mesh_out, mesh_in, self_attn, len_out=None, len_in=None):
        if len_out is not None or len_in is not None:
            # a ragged batch: refused here for batch-free / periodic operators, before any shape check
            if not self._batched:
                self._no_lengths()
            return ops.MeshPlan(self._metric, mesh_out, mesh_in, self.locality, self_attn, len_out=len_out, len_in=len_in)
        if self._batched and ops.mixed_pair(mesh_out, mesh_in) is not None:
            # one mesh shared by the batch against per-sample clouds: rebuilt per call, like every per-sample plan
            return ops.MeshPlan(self._metric, mesh_out, mesh_in, self.locality, self_attn)
        # (self attention on ONE (L, space_dim) mesh shared by the batch is the batch-free layer: the cached plan below)
        if self._batched and not (self_attn and mesh_out is mesh_in and mesh_out.dim() == 2):
            if mesh_out.dim() != 3:
                raise RuntimeError(f"{type(self).__name__} expects (batch, L, space_dim) meshes")
            return ops.MeshPlan(self._metric, mesh_out, mesh_in, self.locality, self_attn)
        if mesh_out.dim() != 2:
            raise RuntimeError(f"{type(self).__name__} expects batch-free (L, space_dim) meshes")
        key = (mesh_out.data_ptr(), mesh_in.data_ptr(), tuple(mesh_out.shape), tuple(mesh_in.shape),
               mesh_out._version, mesh_in._version, float(self.locality), bool(self_attn), mesh_out.device.index)
        plan = self._plans.get(key)
        if plan is None:
            while len(self._plans) >= self._PLAN_CACHE:        # least recently used goes first
                self._plans.popitem(last=False)
            plan = ops.MeshPlan(self._metric, mesh_out, mesh_in, self.locality, self_attn)
            self._plans[key] = plan
        else:
            self._plans.move_to_end(key)
        if ops._capturing():
            ops._pin(plan)        # its buffers' addresses are now baked into a hipGraph: never release them
        return plan

    def _no_lengths(self):
        raise ValueError(f"{type(self).__name__}: lengths are defined for per-sample meshes (posatt / posatt_cross) only - "
                         "a batch-free mesh has no per-sample length")

    def _ragged(self, mesh_out, mesh_in, inputs, len_out, len_in, self_attn, plan=None):
        """The layer on a ragged batch (ops.MeshPlan with lengths -> pit_posatt_ragged_*).  ``plan``: a plan built for exactly
        these meshes, lengths and this locality (pit.processor builds one for all its blocks)."""
        if self._overridden():
            raise NotImplementedError("lengths with an overridden dist2att / convolution")
        if ops.mixed_pair(mesh_out, mesh_in) is not None:
            ops.check_mixed(self._metric, mesh_out, mesh_in, len_out, len_in)      # (a length for the shared side: ValueError)
        elif len_out is None or len_in is None:
            raise ValueError(f"{type(self).__name__}: cross attention on a ragged batch needs both len_out and len_in")
        if plan is None:
            plan = self._plan(mesh_out, mesh_in, self_attn, len_out, len_in)
        return ops.posatt_apply(ops.materialize_coords(inputs), self.lmda, plan, self.n_head, concat=self_attn,
                                mesh_out=mesh_out, mesh_in=mesh_in)

    def _overridden(self) -> bool:
        """True if a subclass replaced ``dist2att`` or ``convolution``: the reference's ``forward`` calls
        ``self.dist2att`` / ``self.convolution`` (pit.py:42-43,68-69), so such a subclass expects its methods to be
        what runs - the fused kernel would silently ignore them."""
        cls = type(self)
        return not (getattr(cls.dist2att, "_pit_fused", False) and getattr(cls.convolution, "_pit_fused", False))

    def _composed(self, mesh_out, mesh_in, inputs):
        # pit.py:42-43 / 68-69 literally, through the (possibly overridden) methods; the dense attention tensor exists
        att = self.dist2att(mesh_out, mesh_in, self.lmda, self.locality)
        return self.convolution(att, ops.materialize_coords(inputs))

    def forward(self, mesh, inputs, lengths=None):
        """``lengths`` (per-sample meshes only): point counts of a ragged batch - sample s is computed from its first
        lengths[s] points alone, rows beyond come out as zeros in the head columns (README, "Ragged batches").
        A 2-d ``mesh`` (L, space_dim) is one mesh shared by the whole batch: what ``posatt_fixed.forward`` computes for it -
        the batch-free plan from this module's LRU cache, the same launches; it has no per-sample length."""
        if lengths is not None:
            lengths = ops.as_lengths(lengths, mesh.device, mesh.shape[0]) if mesh.dim() == 3 else lengths
            return self._ragged(mesh, mesh, inputs, lengths, lengths, True)
        if self._overridden():
            inputs = ops.materialize_coords(inputs)
            return torch.cat((inputs, self._composed(mesh, mesh, inputs)), dim=-1)
        if ops.mesh_grad_wanted(mesh):           # d(mesh) through the layer: refused up front for what it does not cover
            ops._check_mesh_grad(self._metric)
            plan = self._plan(mesh, mesh, True)
            return ops.posatt_apply(ops.materialize_coords(inputs), self.lmda, plan, self.n_head, concat=True,
                                    mesh_out=mesh, mesh_in=mesh)
        plan = self._plan(mesh, mesh, True)
        return ops.posatt_apply(inputs, self.lmda, plan, self.n_head, concat=True)

    def _cross(self, mesh_out, mesh_in, inputs, out_bf16: bool = False, len_out=None, len_in=None):
        if len_out is not None or len_in is not None:
            return self._ragged(mesh_out, mesh_in, inputs, len_out, len_in, False)
        if self._overridden():
            return self._composed(mesh_out, mesh_in, inputs)
        if ops.mesh_grad_wanted(mesh_out, mesh_in):
            # d(mesh) through the layer: no bf16 output, no fused coordinate read - the concat is materialised so that its
            # coordinate channels pass their gradient to mesh_in as well
            ops._check_mesh_grad(self._metric)
            plan = self._plan(mesh_out, mesh_in, False)
            return ops.posatt_apply(ops.materialize_coords(inputs), self.lmda, plan, self.n_head, concat=False,
                                    mesh_out=mesh_out, mesh_in=mesh_in)
        plan = self._plan(mesh_out, mesh_in, False)
        if out_bf16:                             # (pit.decoder, bf16 mode: the result feeds a kaiming_mlp that reads bf16)
            return ops.posatt_apply(ops.materialize_coords(inputs), self.lmda, plan, self.n_head, concat=False, out_bf16=True)
        coords = getattr(inputs, "_pit_coords", None)
        if coords is not None:                   # encoder input tagged by ops.tag_coords: cat((mesh_in, func), -1) not yet built
            kd = mesh_in.shape[-1]
            fused = (plan.nbr_idx is not None and plan.mesh_batch == 1 and coords.shape == mesh_in.shape
                     and coords.data_ptr() == mesh_in.data_ptr())
            if fused:                            # the candidate-list kernels read the coordinate channels from mesh_in
                return ops.posatt_apply(inputs, self.lmda, plan, self.n_head, concat=False, coord_dims=kd)
            inputs = ops.materialize_coords(inputs)
        return ops.posatt_apply(inputs, self.lmda, plan, self.n_head, concat=False)

    # -- dense helpers kept for API compatibility with the reference (not used by forward)
    def dist2att(self, mesh_out, mesh_in, scale, locality, len_out=None, len_in=None):
        """Dense attention weights ((b,)H,L_out,L_in) of pit.py:46-52 for code that inspects them
        (``scale`` is the lmda parameter, as in the reference).  Built by running the fused HIP
        kernel on the identity as values, so it is exactly the matrix ``forward`` applies - there
        is no second, eager implementation of the mask/softmax; ``forward`` never builds it.
        ``len_out`` / ``len_in`` (ragged batches): padded rows and padded keys of the matrix are zero."""
        if len_out is not None or len_in is not None:
            if not self._batched:
                self._no_lengths()
            if ops.mixed_pair(mesh_out, mesh_in) is not None:
                ops.check_mixed(self._metric, mesh_out, mesh_in, len_out, len_in)
            elif len_out is None or len_in is None:
                raise ValueError("dist2att on a ragged batch needs both len_out and len_in")
            plan = ops.MeshPlan(self._metric, mesh_out, mesh_in, float(locality), False, len_out=len_out, len_in=len_in)
            eye = torch.eye(plan.n_in, device=mesh_in.device).unsqueeze(0).repeat(plan.mesh_batch, 1, 1)
            att = ops.posatt_apply(eye, scale, plan, self.n_head, concat=False, mesh_out=mesh_out, mesh_in=mesh_in)
            return att.reshape(plan.mesh_batch, plan.n_out, self.n_head, plan.n_in).permute(0, 2, 1, 3)
        if ops.mixed_pair(mesh_out, mesh_in) is not None:
            ops.check_mixed(self._metric, mesh_out, mesh_in)
        if ops.mesh_grad_wanted(mesh_out, mesh_in):
            ops._check_mesh_grad(self._metric)
        plan = ops.MeshPlan(self._metric, mesh_out, mesh_in, float(locality), False)
        eye = torch.eye(plan.n_in, device=mesh_in.device).unsqueeze(0).repeat(plan.mesh_batch, 1, 1)
        att = ops.posatt_apply(eye, scale, plan, self.n_head, concat=False, mesh_out=mesh_out,
                               mesh_in=mesh_in)                                   # (mb, L_out, H*L_in)
        att = att.reshape(plan.mesh_batch, plan.n_out, self.n_head, plan.n_in).permute(0, 2, 1, 3)
        return att if self._batched else att[0]

    def convolution(self, A, U):
        """pit.py:54-57 for a caller-provided dense A (a plain tensor contraction; the fused path has
        no dense A to contract - ``forward`` does not call this)."""
        eq = "bhnj,bjd->bnhd" if self._batched else "hnj,bjd->bnhd"
        # 'high' (pit.py:2) lets ATen use reduced-precision fp32 GEMMs; this helper contracts in fp64 and rounds once
        # (at least as exact as the fused forward) without touching the process-global precision switch
        out = torch.einsum(eq, A.double(), U.double()).to(U.dtype)
        return out.reshape(U.shape[0], -1, self.n_head * U.shape[-1])

    dist2att._pit_fused = True          # (markers: see _overridden)
    convolution._pit_fused = True


class posatt_cross(posatt):
    """Cross attention mesh_in -> mesh_out on per-sample meshes (pit.py:59-71).  Either mesh may be ONE (n, space_dim) mesh
    shared by the whole batch against the other's (batch, n', space_dim) clouds - the broadcast of pit.py:47-48; only the cloud
    side can have a length (README, "A latent mesh shared by the batch")."""

    def forward(self, mesh_out, mesh_in, inputs, out_bf16: bool = False, len_out=None, len_in=None):
        return self._cross(mesh_out, mesh_in, inputs, out_bf16, len_out, len_in)


class posatt_fixed(posatt):
    """Batch-free meshes: one set of weights shared by the batch (pit.py:129-144)."""
    _batched = False


class posatt_cross_fixed(posatt_fixed):
    def forward(self, mesh_out, mesh_in, inputs, out_bf16: bool = False):       # pit.py:151-159
        return self._cross(mesh_out, mesh_in, inputs, out_bf16)


class posatt_periodic1d(posatt_fixed):
    """Periodic 1-d line mesh (pit.py:186-200)."""
    _metric = "periodic1d"


class posatt_cross_periodic1d(posatt_periodic1d):
    def forward(self, mesh_out, mesh_in, inputs, out_bf16: bool = False):       # pit.py:207-215
        return self._cross(mesh_out, mesh_in, inputs, out_bf16)


class posatt_periodic2d(posatt_fixed):
    """Periodic square grid (pit.py:243-258)."""
    _metric = "periodic2d"


class posatt_cross_periodic2d(posatt_periodic2d):
    def forward(self, mesh_out, mesh_in, inputs, out_bf16: bool = False):       # pit.py:265-273
        return self._cross(mesh_out, mesh_in, inputs, out_bf16)


_OWN_CROSS_FORWARDS = tuple(c.forward for c in (posatt_cross, posatt_cross_fixed, posatt_cross_periodic1d, posatt_cross_periodic2d))


class pit(nn.Module):
    """Encoder / processor / decoder assembly (pit.py:73-127).  No ``forward``: the task
    subclasses supply it, exactly as in the reference."""

    def __init_subclass__(cls, **kw):
        # the scripts wrap the model in torch.compile (train_darcy.py:112): the task forward runs eagerly
        # under dynamo (nothing to trace - the operators are hand-written kernels behind ctypes)
        super().__init_subclass__(**kw)
        fwd = getattr(cls, "forward", None)          # own, or inherited from a mixin next to pit in the bases
        if fwd is not None and fwd is not nn.Module.forward and not getattr(fwd, "_pit_eager", False):
            cls.forward = _eager_under_dynamo(fwd)

    def __init__(self, space_dim, in_dim, out_dim, hid_dim, n_head, n_blocks, mesh_ltt, en_loc, de_loc):
        super().__init__()
        self.space_dim = space_dim
        self.in_dim = in_dim
        self.out_dim = out_dim
        self.hid_dim = hid_dim
        self.n_head = n_head
        self.n_blocks = n_blocks
        self.mesh_ltt = mesh_ltt.reshape(-1, self.space_dim) if mesh_ltt is not None else mesh_ltt
        self.en_local = en_loc
        self.de_local = de_loc

        self.down = posatt_cross(self.n_head, self.in_dim, self.en_local)
        self.en_layer = kaiming_mlp(self.n_head * (self.in_dim + self.space_dim), self.hid_dim, self.hid_dim)
        self.conv = nn.ModuleList([posatt(self.n_head, self.hid_dim, 1.0) for _ in range(self.n_blocks)])
        self.mlp = nn.ModuleList([kaiming_mlp((1 + self.n_head) * self.hid_dim, self.hid_dim, self.hid_dim)
                                  for _ in range(self.n_blocks)])
        self.up = posatt_cross(self.n_head, self.hid_dim, self.de_local)
        self.de = kaiming_mlp(self.n_head * self.hid_dim, self.hid_dim, self.out_dim)

    def _mesh_grad(self, *meshes) -> bool:
        """The per-layer path for gradients w.r.t. the meshes: grad mode on and one of ``meshes`` (or ``self.mesh_ltt``) requires
        grad.  Then every attention layer runs on its own (_PosAtt with the meshes as inputs), none of the fused launches does.
        What that path does not cover (periodic metrics, the bf16 math mode) raises here, before anything is launched."""
        if not ops.mesh_grad_wanted(self.mesh_ltt, *meshes):
            # the reproducible mode takes the same per-layer path at the same decision points (bf16 mode: refused here)
            return ops.reproducible_wanted()
        for m in (self.down, *self.conv, self.up):
            if isinstance(m, posatt):
                ops._check_mesh_grad(m._metric)
        ops._check_mesh_grad("euclid")
        return True

    @staticmethod
    def _mlp_gelu(layer, x, concat_heads: int = 0, ordered: bool = False):
        # scripts may replace en_layer / mlp[i] by their own modules (train_elasticity.py:39)
        # (ordered: ragged batches - the weight gradients of OUR MLPs are summed in a fixed order)
        if isinstance(layer, kaiming_mlp):
            return layer(x, out_gelu=True, concat_heads=concat_heads, ordered=ordered)
        return gelu(layer(x))

    def _heads_of_block(self, i: int, width: int) -> int:
        """Heads of processor block i if it is one of OUR self-attention layers consuming ``width`` channels
        (then the producing MLP writes straight into its concat buffer), else 0."""
        if 0 <= i < len(self.conv) and isinstance(self.conv[i], posatt) and self.conv[i].in_dim == width:
            return int(self.conv[i].n_head)
        return 0

    def _swap_attention(self, self_cls, cross_cls):
        """Replace down / conv / up by another geometry's operators AFTER the base layers were
        built, as pit.py:182-184,238-240,296-298 do: the extra ``torch.rand`` draws keep the
        RNG stream - and therefore seed-for-seed initialisation - identical to the reference."""
        self.down = cross_cls(self.n_head, self.in_dim, self.en_local)
        self.conv = nn.ModuleList([self_cls(self.n_head, self.hid_dim, 1.0) for _ in range(self.n_blocks)])
        self.up = cross_cls(self.n_head, self.hid_dim, self.de_local)

    @staticmethod
    def _plain(*modules) -> bool:
        """None of the modules is hooked or has its forward patched on the instance (those expect to be CALLED: no fusing)."""
        for m in modules:
            if "forward" in m.__dict__ or m._forward_pre_hooks or m._backward_hooks or m._backward_pre_hooks \
                    or any(not getattr(f, "_pit_internal", False) for f in m._forward_hooks.values()):
                return False
        return True

    def _edge_modules(self, att, mlp) -> bool:
        """Cross-attention ``att`` and kaiming_mlp ``mlp`` are OUR unmodified modules of a shape the fused launches cover."""
        return bool(ops.EDGE_FUSION and isinstance(att, posatt) and not att._batched and type(att).forward in _OWN_CROSS_FORWARDS
                    and not att._overridden() and type(mlp) is kaiming_mlp and mlp.mlp1.bias is not None and mlp.mlp2.bias is not None
                    and self._plain(att, mlp, mlp.mlp1, mlp.mlp2) and mlp.mlp1.out_features in (32, 64) and att.n_head in (1, 2))

    def _edge_layer(self, att, mlp, mesh_out, mesh_in, batch, device, needs_union):
        """The mesh plan when cross-attention ``att`` followed by kaiming_mlp ``mlp`` can run as one fused launch per direction
        (ops.encoder_apply / ops.decoder_apply: batch-free meshes, small regime), else None."""
        if not self._edge_modules(att, mlp):
            return None
        if not (torch.is_tensor(mesh_out) and torch.is_tensor(mesh_in) and mesh_out.dim() == 2 and mesh_in.dim() == 2
                and mesh_out.is_cuda and mesh_in.is_cuda and mesh_out.device == device and mesh_in.device == device):
            return None
        if mlp.mlp1.out_features not in (32, 64) or att.n_head not in (1, 2):
            return None
        plan = att._plan(mesh_out, mesh_in, False)
        return plan if ops.edge_fusion_supported(plan, att.n_head, mlp.mlp1.out_features, batch, needs_union) else None

    def _fused_encoder(self, mesh_in, func_in, mesh_ltt, early):
        """gelu(en_layer(down(...))) as ONE launch per direction (ops.encoder_apply), or None: run the two modules."""
        if not (torch.is_tensor(func_in) and func_in.is_cuda and func_in.dim() == 3 and func_in.dtype == torch.float32):
            return None
        if torch.is_grad_enabled() and func_in.requires_grad:         # (the fused backward gives the input data no gradient)
            return None
        en, down = self.en_layer, self.down
        if type(en) is not kaiming_mlp or en.mlp1.out_features != en.mlp2.out_features:
            return None
        coords = getattr(func_in, "_pit_coords", None)
        kd = 0
        if coords is not None:
            if not (torch.is_tensor(mesh_in) and coords.shape == mesh_in.shape and coords.data_ptr() == mesh_in.data_ptr()):
                return None
            kd = mesh_in.shape[-1]
        chans = kd + func_in.shape[-1]
        if chans > 8 or down.n_head * chans > 16 or en.mlp1.in_features != down.n_head * chans:
            return None
        plan = self._edge_layer(down, en, mesh_ltt, mesh_in, func_in.shape[0], func_in.device, False)
        if plan is None or plan.n_in != func_in.shape[1]:
            return None
        return ops.encoder_apply(func_in, down.lmda, plan, down.n_head, (en.mlp1.weight, en.mlp1.bias, en.mlp2.weight, en.mlp2.bias),
                                 concat_heads=self._heads_of_block(0, self.hid_dim), early=early)

    def _cached_decoder_plan(self, mesh_ltt, batch, device):
        """The plan the fused decoder ran on last time, if this forward's decoder will - as far as the encoder can tell: same
        latent mesh - run on it again; its weights are then formed under the encoder-side launch (ops.early_decoder_weights).
        A wrong guess costs nothing but the unused tiles: ops.decoder_apply checks plan and lmda before it uses them."""
        up, de = self.up, self.de
        if not (isinstance(up, posatt) and up._plans and torch.is_tensor(mesh_ltt) and mesh_ltt.dim() == 2 and self._edge_modules(up, de)):
            return None
        hid = self.hid_dim
        if de.mlp2.out_features > 4 or de.mlp1.out_features != hid or de.mlp1.in_features != up.n_head * hid:
            return None
        # (the cache is keyed on the CALLER's mesh tensors - posatt._plan: address, shape, version - the plan may hold copies)
        key, plan = next(reversed(up._plans.items()))
        if key[1] != mesh_ltt.data_ptr() or key[3] != tuple(mesh_ltt.shape) or key[5] != mesh_ltt._version or key[8] != device.index:
            return None
        return plan if ops.edge_fusion_supported(plan, up.n_head, hid, batch, True) else None

    def _ragged_lengths(self, meshes, **lengths):
        """Lengths of a ragged batch as device tensors; None when no length was given."""
        if all(v is None for v in lengths.values()):
            return None
        mesh = next((m for m in meshes if torch.is_tensor(m) and m.dim() == 3), None)      # (a mixed pair: the cloud side)
        if mesh is None:
            raise ValueError("lengths need per-sample (batch, n, space_dim) meshes: a batch-free mesh has no per-sample length")
        return tuple(None if v is None else ops.as_lengths(v, mesh.device, mesh.shape[0]) for v in lengths.values())

    def encoder(self, mesh_in, func_in, mesh_ltt, len_in=None, len_ltt=None):
        """``len_in`` / ``len_ltt`` (keywords; ragged batches of per-sample clouds): point counts of ``mesh_in`` and
        ``mesh_ltt``.  With lengths every layer runs on its own on the ragged kernels.  A 2-d ``mesh_ltt`` is one latent mesh
        shared by the whole batch: it has no length (``len_ltt`` must stay None) and the result has no padded rows."""
        rag = self._ragged_lengths((mesh_in, mesh_ltt), len_in=len_in, len_ltt=len_ltt)
        if rag is not None:
            len_in, len_ltt = rag
            if ops.mixed_pair(mesh_ltt, mesh_in) is not None:
                ops.check_mixed(getattr(self.down, "_metric", "euclid"), mesh_ltt, mesh_in, len_ltt, len_in)
            elif len_in is None or len_ltt is None:
                raise ValueError("encoder: a ragged batch needs both len_in and len_ltt")
            return self._mlp_gelu(self.en_layer, self.down(mesh_ltt, mesh_in, func_in, len_out=len_ltt, len_in=len_in), ordered=True)
        if self._mesh_grad(mesh_in, mesh_ltt):
            return self._mlp_gelu(self.en_layer, self.down(mesh_ltt, mesh_in, func_in), self._heads_of_block(0, self.hid_dim))
        # the fused processor's weights depend on (mesh_ltt, lmda) only: they are formed by extra workgroups of the
        # encoder-side launch (ops.early_block_weights) instead of a launch of their own; processor() picks them up
        early = None
        try:
            if ops.EARLY_WEIGHTS != "0" and torch.is_tensor(func_in) and func_in.is_cuda and func_in.dim() >= 2:
                plan = self._fused_plan(mesh_ltt, func_in.shape[0], self.hid_dim, func_in.device)
                if plan is not None:
                    need_q = torch.is_grad_enabled() and (func_in.requires_grad or any(q.requires_grad for q in self.parameters()))
                    early = ops.early_block_weights(plan, [a.lmda for a in self.conv], self.conv[0].n_head, need_q)
            if ops.EDGE_FUSION and torch.is_tensor(func_in) and func_in.is_cuda and func_in.dim() == 3:
                dplan = self._cached_decoder_plan(mesh_ltt, func_in.shape[0], func_in.device)
                if dplan is not None:
                    need_q = torch.is_grad_enabled() and any(q.requires_grad for q in self.parameters())
                    ops.early_decoder_weights(dplan, self.up.lmda, self.up.n_head, need_q, self.de.mlp1.weight)
            fused = self._fused_encoder(mesh_in, func_in, mesh_ltt, early)
            func_ltt = self.down(mesh_ltt, mesh_in, func_in) if fused is None else None
            if early is not None:
                early.join()
        finally:
            ops.drop_forward_job(early)          # (a call that raised must not leave its job armed for the thread's next layer)
        out = fused if fused is not None else self._mlp_gelu(self.en_layer, func_ltt, self._heads_of_block(0, self.hid_dim))
        if early is not None:
            # the handle travels ON the activation tensor to the processor call that consumes it (no module state: an encoder
            # call that is not followed by a processor call keeps nothing alive beyond its own result, and an unrelated
            # processor call can never pick up a stale handle - VERDICT r5 weak 9)
            out._pit_early = early
        return out

    def _fused_processor(self, func_ltt, mesh_ltt):
        """The fused block kernels (ops.processor_apply) when every block is one of OUR batch-free self-attention
        layers followed by a kaiming_mlp of the standard shape, nothing is hooked or overridden and the shape is in
        the small regime; None = run the blocks one by one."""
        early = getattr(func_ltt, "_pit_early", None) if torch.is_tensor(func_ltt) else None
        if not (func_ltt.is_cuda and func_ltt.dim() == 3 and func_ltt.dtype == torch.float32):
            return None
        plan = self._fused_plan(mesh_ltt, func_ltt.shape[0], func_ltt.shape[-1], func_ltt.device, func_ltt.shape[1])
        if plan is None:
            return None
        return ops.processor_apply(func_ltt, plan, self.conv[0].n_head, [a.lmda for a in self.conv],
                                   [(w.mlp1.weight, w.mlp1.bias, w.mlp2.weight, w.mlp2.bias) for w in self.mlp], early=early)

    def _fused_plan(self, mesh_ltt, batch, hid, device, n_pts=None):
        """The latent mesh plan of the fused processor for activations (batch, n_pts, hid) on `device`, or None when the
        blocks have to run one by one."""
        n = len(self.conv)
        # (pit_block_weights forms the weights of at most 16 blocks in its one launch: deeper processors - the reference accepts
        # any n_blocks - run block by block)
        if not (ops.BLOCK_FUSION and 0 < n <= ops.BLOCK_MAX_LAYERS and n == len(self.mlp) and torch.is_tensor(mesh_ltt) and mesh_ltt.dim() == 2
                and device.type == "cuda" and mesh_ltt.device == device):
            return None
        heads = self.conv[0].n_head
        kinds = (posatt, posatt_fixed, posatt_periodic1d, posatt_periodic2d)      # (posatt: on a 2-d mesh it is posatt_fixed)
        for a, w in zip(self.conv, self.mlp):
            if type(a) not in kinds or type(a) is not type(self.conv[0]) or a.locality != 1.0 or a.n_head != heads \
                    or a.in_dim != hid or type(w) is not kaiming_mlp:
                return None
            if tuple(w.mlp1.weight.shape) != (hid, (1 + heads) * hid) or tuple(w.mlp2.weight.shape) != (hid, hid) \
                    or w.mlp1.bias is None or w.mlp2.bias is None:
                return None
            if "forward" in a.__dict__ or "forward" in w.__dict__:      # forward patched on the instance: it must be called
                return None
            for m in (a, w, w.mlp1, w.mlp2):            # hooks expect the modules to be CALLED
                if any(not getattr(f, "_pit_internal", False) for f in m._forward_hooks.values()) \
                        or m._forward_pre_hooks or m._backward_hooks or m._backward_pre_hooks:
                    return None
        if (n_pts is not None and mesh_ltt.shape[0] != n_pts) or not ops.block_fusion_supported(mesh_ltt.shape[0], heads, hid, batch,
                                                                                                      mesh_ltt.shape[-1]):
            return None
        return self.conv[0]._plan(mesh_ltt, mesh_ltt, True)

    def _precomputed_weights(self, func_ltt, mesh_ltt):
        """Large regime, batch-free meshes (round 4): the softmax weights of every block - functions of (mesh_ltt, lmda) only -
        from ONE launch, read by the attention launches instead of re-formed in every workgroup.  None = not applicable."""
        n = len(self.conv)
        if not (ops.PRE_WEIGHTS and n and torch.is_tensor(mesh_ltt) and mesh_ltt.dim() == 2 and torch.is_tensor(func_ltt)
                and func_ltt.is_cuda and func_ltt.dim() == 3 and func_ltt.dtype == torch.float32):
            return None
        hid, heads = func_ltt.shape[-1], self.conv[0].n_head
        kinds = (posatt, posatt_fixed, posatt_periodic1d, posatt_periodic2d)      # (posatt: on a 2-d mesh it is posatt_fixed)
        for a in self.conv:
            if type(a) not in kinds or type(a) is not type(self.conv[0]) or a.locality != 1.0 or a.n_head != heads or a.in_dim != hid \
                    or "forward" in a.__dict__ or a._forward_hooks or a._forward_pre_hooks or a._backward_hooks or a._backward_pre_hooks:
                return None
        if mesh_ltt.shape[0] != func_ltt.shape[1] or not ops.pre_weights_supported(mesh_ltt.shape[0], heads, hid, func_ltt.shape[0],
                                                                                                 mesh_ltt.shape[-1]):
            return None
        plan = self.conv[0]._plan(mesh_ltt, mesh_ltt, True)
        need_q = torch.is_grad_enabled() and any(a.lmda.requires_grad for a in self.conv)
        return ops.block_weights(plan, [a.lmda for a in self.conv], heads, need_q)

    def processor(self, func_ltt, mesh_ltt, len_ltt=None):
        rag = self._ragged_lengths((mesh_ltt,), len_ltt=len_ltt)
        if rag is not None:
            # one plan (selection statistics of mesh_ltt under these lengths) for all blocks that are OUR layers of one locality
            own = [a for a in self.conv if type(a) is posatt and "forward" not in a.__dict__ and not a._overridden()]
            shared = own[0]._plan(mesh_ltt, mesh_ltt, True, rag[0], rag[0]) if len(own) > 1 else None
            for a, w in zip(self.conv, self.mlp):
                if shared is not None and a in own and a.locality == own[0].locality:
                    func_ltt = a._ragged(mesh_ltt, mesh_ltt, func_ltt, rag[0], rag[0], True, plan=shared)
                else:
                    func_ltt = a(mesh_ltt, func_ltt, lengths=rag[0])
                func_ltt = self._mlp_gelu(w, func_ltt, ordered=True)
            return func_ltt
        if self._mesh_grad(mesh_ltt):
            for i, (a, w) in enumerate(zip(self.conv, self.mlp)):
                func_ltt = self._mlp_gelu(w, a(mesh_ltt, func_ltt), self._heads_of_block(i + 1, self.hid_dim))
            return func_ltt
        fused = self._fused_processor(func_ltt, mesh_ltt)
        if fused is not None:
            return fused
        weights = self._precomputed_weights(func_ltt, mesh_ltt)
        if torch.is_tensor(func_ltt) and func_ltt.is_cuda and func_ltt.dim() == 3 and ops.get_math_mode() == "bf16":
            # bf16 mode: the one-launch MLP chains read bf16 copies of the weights - all blocks' in one launch, here
            ops.prepare_chain_weights([(w.mlp1.weight, w.mlp2.weight) for w in self.mlp if type(w) is kaiming_mlp],
                                      func_ltt.shape[0] * func_ltt.shape[1])
        for i, (a, w) in enumerate(zip(self.conv, self.mlp)):
            if weights is not None:
                func_ltt = ops.posatt_pre_apply(func_ltt, a.lmda, weights, i, a.n_head)
                func_ltt = self._mlp_gelu(w, func_ltt, self._heads_of_block(i + 1, self.hid_dim))
                continue
            func_ltt = a(mesh_ltt, func_ltt)
            func_ltt = self._mlp_gelu(w, func_ltt, self._heads_of_block(i + 1, self.hid_dim))
        return func_ltt

    def _folded_decoder(self, mesh_ltt, func_ltt, mesh_out):
        """de(up(...)) with de.mlp1 folded into the values, or None: modules that are not OUR unmodified ones, hooks, an output
        wider than 4 channels, widths the kernels do not cover, fewer than twice as many output as latent points (the fold moves
        a Linear from the n_out rows to the n_in rows: nothing to gain), two heads on meshes without a fold plan."""
        de, up = self.de, self.up
        if not (ops.FOLD_DECODER and torch.is_tensor(func_ltt) and func_ltt.is_cuda and func_ltt.dim() == 3
                and func_ltt.dtype == torch.float32 and torch.is_tensor(mesh_out) and torch.is_tensor(mesh_ltt)):
            return None
        if not (isinstance(up, posatt) and type(up).forward in _OWN_CROSS_FORWARDS and not up._overridden() and type(de) is kaiming_mlp
                and de.mlp1.bias is not None and de.mlp2.bias is not None and self._plain(up, de, de.mlp1, de.mlp2)):
            return None
        hid, heads = func_ltt.shape[-1], up.n_head
        if not (de.mlp2.out_features <= 4 and de.mlp1.out_features == hid and de.mlp1.in_features == heads * hid
                and hid in (64, 128, 256) and heads in (1, 2)):
            return None
        n_out, n_in = mesh_out.shape[-2], mesh_ltt.shape[-2]
        if n_out < 2 * n_in or n_in != func_ltt.shape[1] or mesh_out.dim() != (3 if up._batched else 2) or mesh_ltt.dim() != mesh_out.dim():
            return None
        if mesh_out.device != func_ltt.device or mesh_ltt.device != func_ltt.device:
            return None
        plan = up._plan(mesh_out, mesh_ltt, False)
        fold_att = (not up._batched) and ops.fold_att_supported(plan, heads, hid, func_ltt.shape[0])
        if not fold_att and heads != 1:
            return None
        return ops.fold_decoder_apply(func_ltt, up.lmda, plan, heads, (de.mlp1.weight, de.mlp1.bias, de.mlp2.weight, de.mlp2.bias),
                                      fold_att)

    def decoder(self, mesh_ltt, func_ltt, mesh_out, len_ltt=None, len_out=None):
        rag = self._ragged_lengths((mesh_ltt, mesh_out), len_ltt=len_ltt, len_out=len_out)
        if rag is not None:
            len_ltt, len_out = rag
            if ops.mixed_pair(mesh_out, mesh_ltt) is not None:
                ops.check_mixed(getattr(self.up, "_metric", "euclid"), mesh_out, mesh_ltt, len_out, len_ltt)
            elif len_ltt is None or len_out is None:
                raise ValueError("decoder: a ragged batch needs both len_ltt and len_out")
            f = self.up(mesh_out, mesh_ltt, func_ltt, len_out=len_out, len_in=len_ltt)
            return self.de(f, ordered=True) if isinstance(self.de, kaiming_mlp) else self.de(f)
        # bf16 mode (BASELINE configs 3 and 5): the up-projection's output - the largest tensor of the model, rows x H*hid -
        # and with it the decoder MLP's saved activations and their gradients are kept in memory as bf16 when the
        # decoder MLP's shape runs on the kernels that read them (ops.mlp_bf16_io_supported); fp32 accumulation throughout
        de, up = self.de, self.up
        if self._mesh_grad(mesh_ltt, mesh_out):
            return de(up(mesh_out, mesh_ltt, func_ltt))
        # small regime on batch-free meshes: up-projection + decoder MLP as ONE launch per direction (every math mode: the
        # launch is latency-bound and contracts in fp32, like the fused processor blocks)
        if torch.is_tensor(func_ltt) and func_ltt.is_cuda and func_ltt.dim() == 3 and func_ltt.dtype == torch.float32 \
                and type(de) is kaiming_mlp and isinstance(up, posatt) and de.mlp2.out_features <= 4 \
                and de.mlp1.out_features == func_ltt.shape[-1] and de.mlp1.in_features == up.n_head * func_ltt.shape[-1]:
            plan = self._edge_layer(up, de, mesh_out, mesh_ltt, func_ltt.shape[0], func_ltt.device, True)
            if plan is not None and func_ltt.shape[0] * plan.n_out >= ops.FOLD_EDGE_ROWS:
                # many rows: the folded decoder (below) moves de.mlp1 to the latent points and adds d(values) once per TALL slab
                folded = self._folded_decoder(mesh_ltt, func_ltt, mesh_out)
                if folded is not None:
                    return folded
            if plan is not None and plan.n_in == func_ltt.shape[1]:
                return ops.decoder_apply(func_ltt, up.lmda, plan, up.n_head,
                                         (de.mlp1.weight, de.mlp1.bias, de.mlp2.weight, de.mlp2.bias))
        # round 6: de.mlp1 folded into the values (ops.fold_decoder_apply): nothing non-linear sits between `up` and `de.mlp1`, so the
        # first Linear runs on the latent points and the (batch, n_out, H*hid) tensor below never exists
        folded = self._folded_decoder(mesh_ltt, func_ltt, mesh_out)
        if folded is not None:
            return folded
        if type(de) is kaiming_mlp and isinstance(up, posatt) and type(up).forward in _OWN_CROSS_FORWARDS and func_ltt.is_cuda \
                and ops.get_math_mode() == "bf16" and torch.is_tensor(mesh_out) and not up._forward_hooks and not de._forward_hooks:
            rows = func_ltt.shape[0] * mesh_out.shape[-2]
            if ops.mlp_bf16_io_supported(rows, de.mlp1.in_features, de.mlp1.out_features, de.mlp2.out_features):
                return de(up(mesh_out, mesh_ltt, func_ltt, out_bf16=True))
        func_out = self.up(mesh_out, mesh_ltt, func_ltt)
        return self.de(func_out)


class pit_fixed(pit):
    """pit with batch-free Euclidean meshes (pit.py:161-184)."""

    def __init__(self, space_dim, in_dim, out_dim, hid_dim, n_head, n_blocks, mesh_ltt, en_loc, de_loc):
        super().__init__(space_dim, in_dim, out_dim, hid_dim, n_head, n_blocks, mesh_ltt, en_loc, de_loc)
        self._swap_attention(posatt_fixed, posatt_cross_fixed)


class pit_periodic1d(pit):
    """pit on a periodic line mesh (pit.py:217-240)."""

    def __init__(self, space_dim, in_dim, out_dim, hid_dim, n_head, n_blocks, mesh_ltt, en_loc, de_loc):
        super().__init__(space_dim, in_dim, out_dim, hid_dim, n_head, n_blocks, mesh_ltt, en_loc, de_loc)
        self._swap_attention(posatt_periodic1d, posatt_cross_periodic1d)


class pit_periodic2d(pit):
    """pit on a periodic square grid (pit.py:275-298)."""

    def __init__(self, space_dim, in_dim, out_dim, hid_dim, n_head, n_blocks, mesh_ltt, en_loc, de_loc):
        super().__init__(space_dim, in_dim, out_dim, hid_dim, n_head, n_blocks, mesh_ltt, en_loc, de_loc)
        self._swap_attention(posatt_periodic2d, posatt_cross_periodic2d)
