"""CPU stand-in for Operator built on the oracle — TEST INFRASTRUCTURE ONLY.

Lets the multi-process (gloo, CPU) tests exercise ShardedOperator's sharding, all-gather and
all-reduce logic without a GPU.  Same call semantics as Operator for static grids and for
dynamic grids paired view-by-view with time slices; differentiable through a torch autograd
Function whose backward is the oracle adjoint.
"""
import math
import os
import sys

import numpy as np
import torch as tr

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle  # noqa: E402
from sph_raytracer_amd.raytracer import _layout_for, find_starts  # noqa: E402


class _Fn(tr.autograd.Function):
    @staticmethod
    def forward(ctx, density, op):
        ctx.op = op
        ctx.shape = density.shape
        return op._fwd(density.detach())

    @staticmethod
    def backward(ctx, g):
        return ctx.op._adj(g, ctx.shape), None


class CpuOperator:
    def __init__(self, grid, geom, device='cpu', reverse=False):
        """reverse: the same matrix with its segments stored in the opposite order, so that
        every row sum of the forward and every column sum of the adjoint (both accumulate in
        storage order) adds its terms last to first: the same operator up to rounding
        (tests/gd_cases.py measures a loop's sensitivity to summation order with it)."""
        self.grid, self.geom, self.device = grid, geom, device
        xs, rays = geom.ray_starts, geom.rays
        shape = tuple(tr.broadcast_shapes(xs.shape, rays.shape))[:-1]
        self.ray_shape = shape
        g = oracle.Grid.from_boundaries(grid.r_b.numpy(), grid.e_b.numpy(), grid.a_b.numpy())
        starts = find_starts(grid, xs).numpy()
        self.ptr, self.vox, self.seg = oracle.trace_segments(g, xs.numpy(), rays.numpy(), starts)
        self.n_vox = math.prod(grid.shape[-3:])
        # the system matrix as float64 triplets (ray, voxel, length) in storage order
        self.ray = np.repeat(np.arange(len(self.ptr) - 1), np.diff(self.ptr))
        if reverse:
            self.ray, self.vox, self.seg = (np.ascontiguousarray(a[::-1])
                                            for a in (self.ray, self.vox, self.seg))
        self.reverse = reverse

    def __call__(self, density):
        return _Fn.apply(tr.as_tensor(density), self)

    def _fwd(self, density):
        n_chan, div, out_shape = _layout_for(self.grid, self.ray_shape, density.shape)
        if self.reverse:    # (np.bincount adds in storage order: each row last segment first)
            dens = density.numpy().astype(np.float64).reshape(-1, self.n_vox)
            n = len(self.ptr) - 1
            if div:
                out = np.bincount(self.ray, dens[self.ray // div, self.vox] * self.seg,
                                  minlength=n)
            else:
                out = np.stack([np.bincount(self.ray, dc[self.vox] * self.seg, minlength=n)
                                for dc in dens])
        else:
            out = oracle.forward(self.ptr, self.vox, self.seg, density.numpy(), self.n_vox,
                                 ray_chan_div=div)
        return tr.from_numpy(np.ascontiguousarray(out).reshape(out_shape)).to(density.dtype)

    def _adj(self, y, dshape):
        n_chan, div, _ = _layout_for(self.grid, self.ray_shape, dshape)
        dtype = y.dtype
        y = y.detach().numpy().reshape(n_chan if not div else 1, -1)
        ray = self.ray
        if div:
            vol = np.zeros((dshape[0], self.n_vox))
            np.add.at(vol, (ray[...] // div, self.vox), y[0][ray] * self.seg)
        else:
            vol = np.stack([np.bincount(self.vox, yc[ray] * self.seg, minlength=self.n_vox)
                            for yc in y])
        return tr.from_numpy(vol.reshape(dshape)).to(dtype)

    def T(self, y):
        return self._adj(tr.as_tensor(y), tuple(self.grid.shape))

    def _apply_adjoint(self, y, dshape, ddtype, ddevice):
        """Operator._apply_adjoint's contract (any grid, dynamic included)."""
        return self._adj(tr.as_tensor(y), tuple(dshape)).to(device=ddevice, dtype=ddtype)
