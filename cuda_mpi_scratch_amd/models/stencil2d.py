"""2D domain-decomposed stencil workload.

Reference: stencil2d/mpi-2d-stencil-subarray{.cpp,-cuda.cu} + stencil2d/stencil2D.h:
a periodic Cartesian grid of ranks, one tile per rank with a ghost ring of
``stencilWidth/2`` cells, halo exchange with subarray datatypes, and an empty
Compute() (the loop ran once). Here the loop is real:

    for it in iters:  halo exchange (8 neighbours, per-peer RCCL messages over xGMI)
                      + 5-point Jacobi (or (2R+1)^2 box) update, double-buffered

driven by the native C++ ``StencilSolver`` on GPU (HIP kernels, RCCL, compute/comm
overlap on two HIP streams, hipGraph replay) and by a torch/gloo reference path
on CPU. ``init="rank"`` reproduces the reference's observable run exactly (tile
filled with -1, core = rank id, one exchange, per-rank dump files).

Usage (one process per GPU):
    torchrun --nproc-per-node 8 -m cuda_mpi_scratch_amd.models.stencil2d --global 32768x32768 --dims 2x4
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import time
from dataclasses import asdict, dataclass, field

import torch

from .. import ops
from .._native import core, hip
from ..parallel import DistContext, TorchHalo, choose_dims, init as dist_init, make_plan, make_rccl_comm
from ..parallel.cart import Decomposition
from ..utils import summarize

_DTYPES = {"f32": torch.float32, "f64": torch.float64}


@dataclass
class StencilConfig:
    global_width: int = 8192
    global_height: int = 8192
    dims: str | None = None          # "RxC"; default MPI_Dims_create-like
    prefer: str = "wide"             # rows <= cols when dims is not given (8 -> 2x4)
    periodic: bool = True
    dtype: str = "f32"
    kind: str = "jacobi5"            # jacobi5 | box
    stencil_width: int = 3           # ghost ring = stencil_width // 2 (reference default 5 -> 2)
    box_weights: list = field(default_factory=list)
    c_center: float = 0.2
    c_neighbor: float = 0.2
    # c_center == c_neighbor: let the time-blocked GPU kernels run the sum form
    # (plain 5-point sums per level, c^S applied once per pass: ~20% faster,
    # equal to the per-step evaluation up to a few ulp). False: per-step
    # evaluation, bitwise equal to S single steps and to the CPU paths.
    sum_form: bool = True
    backend: str = "auto"            # auto | rccl | ipc | local | torch
    overlap: bool | None = None      # None = auto (on only for time_block 1 on unshared GPUs)
    graph: bool = True
    loopback: bool = False           # single GPU: send self-neighbour halos through RCCL
    variant: str = "auto"            # stencil kernel variant: auto | roll | lds
    fuse_periodic: bool = True       # 1x1 periodic: fuse the self-exchange into the kernel addressing
    # Jacobi iterations per halo exchange and per temporally blocked pass on GPU
    # (wave-streaming kernels); the ghost ring is made this deep. 1 = one
    # exchange per iteration; 0 = the measured optimum for the tile
    # (kernels::auto_time_block: fp32 20 on the two-stage pipeline, fp64 16 in
    # the sum form, else 12;
    # docs/PERF.md). Up to 32 for fp32 without overlap, else capped at 16.
    time_block: int = 0
    # periodic=False on GPU: keep the time block (computed as for a periodic
    # grid, the automatic default included) instead of one exchange per
    # iteration. Each pass then runs the tile's interior, S cells away from the
    # fixed edges, on the usual kernels and the frame along them on the
    # held-side kernel (ops.stencil5_tb_held), which keeps the boundary values
    # in the ghost ring fixed at every level. With sum_form=False the result is
    # bitwise the one-exchange-per-iteration one.
    block_fixed_edges: bool = False
    # "chebyshev": every block of M iterations is one M-point Chebyshev cycle of
    # the Jacobi relaxation (ops.chebyshev_cycle: level l of a pass runs its own
    # coefficient pair), which reaches a tolerance in 10-30x fewer sweeps than
    # plain Jacobi. Needs jacobi5 and periodic=False; on GPU also
    # block_fixed_edges and a time block with level kernels (fp32 20 / 24, fp64
    # 12 / 16; time_block=0 picks 24 / 16). The cycle is the unit of progress:
    # run(K) needs K % M == 0 and the field is only meaningful at cycle ends.
    # fp32 stalls at a rounding floor (docs/ARCHITECTURE.md); use f64 for tight
    # tolerances. "none": plain Jacobi.
    relaxation: str = "none"
    # This solver takes a source term, u' = A u + g (Stencil2D.set_source): the
    # Poisson problem. One cycle with a source is the homogeneous level-table
    # pass plus a correction G, built once per set_source, added where the pass
    # stores (docs/ARCHITECTURE.md "Source term"). Needs, on every backend,
    # jacobi5, periodic=False, block_fixed_edges and a time block with level
    # kernels (fp32 20 / 24, fp64 12 / 16; time_block=0 picks 24 / 16). With
    # relaxation="none" the passes run a uniform level table of time_block
    # levels (plain Jacobi). Either way the per-step form runs, the cycle is the
    # unit of progress (run(K) needs K % M == 0) and the field is the iterate at
    # cycle ends only.
    source: bool = False
    seed: int = 1234
    init: str = "random"             # random | rank
    graph_supersteps: int = 0        # super-steps per hipGraph launch (0 = auto, ~1 ms of work)
    # Device-initiated halo — each pass's output bands are pushed tile-to-tile
    # into the neighbours' ghost rings (no pack / wire / unpack launches).
    # None / True = on whenever the backend is ipc (ranks sharing a GPU; the IPC
    # backend refuses ranks on different GPUs unless MXS_IPC_CROSS_DEVICE=1).
    # "validate": RCCL or IPC backend, ranks on any GPUs: prepare() compares one
    # direct push with one backend exchange bitwise on every rank and times both
    # openings; direct runs only if equal everywhere and faster (agreed).
    direct_halo: bool | str | None = None
    # What moves the direct halo's bands: "kernel" (a CU push kernel) or
    # "copy-engine" (hipMemcpy2DAsync on the SDMA engines, no CU).
    direct_engine: str = "kernel"
    # Opening super-step of a call with peers (RCCL): its priming exchange runs
    # under the chunks that read only core cells ("interior-first") or before
    # the pass ("serial"). "auto" (default): prepare() times both on every rank
    # in paired rounds, agrees the per-round maxima over ranks (the window is
    # the max over ranks) and keeps interior-first when the median ratio of the
    # maxima is below 1 - min_gain with 95% confidence (runtime/decision.hpp).
    opening: str = "auto"
    min_gain: float = 0.0
    # Super-steps after an interior-first opening: "serial" (pass, then the
    # exchange of its output), "interior-first" (each super-step like the
    # opening), or "auto" (prepare() of a call with >= 2 super-steps times both
    # and all ranks adopt the faster).
    steady: str = "auto"
    # Single GPU with loopback: follow the peers' schedule (every call primes,
    # the last pass of a call is bare, the opening is chosen as with peers), so
    # one GPU rehearses the window an N-GPU run executes.
    rehearse_peers: bool = False
    # RCCL backend: the halo exchange on its own communicator whose kernels use
    # at most this many workgroups (0 = RCCL's default): the interior-first
    # opening's exchange runs on the 32-48 CUs the inner launch leaves free.
    halo_max_ctas: int = 0
    # One-GPU rehearsal (loopback, rehearse_peers): every RCCL transfer is
    # followed by a single-wave kernel holding the stream this long (us), in
    # place of the xGMI wire time the loopback does not have.
    wire_delay_us: float = 0.0
    # HIP stream priorities of the solver's main (exchange chain) and side streams.
    main_priority: int = -1
    side_priority: int = 0
    # Super-steps estimated longer than this run from eager launches, not a
    # hipGraph (long passes: eager measured faster). 0 = always graphs.
    graph_max_superstep_us: float = 150.0

    # The string options and their allowed values (checked at construction, so a
    # typo fails here on every rank instead of deep in the native solver).
    _CHOICES = {"prefer": ("wide", "mpi"), "dtype": tuple(_DTYPES), "kind": ("jacobi5", "box"),
                "backend": ("auto", "rccl", "ipc", "local", "torch"), "variant": ("auto", "roll", "lds"),
                "init": ("random", "rank"), "direct_engine": ("kernel", "copy-engine"),
                "opening": ("auto", "serial", "interior-first"), "steady": ("auto", "serial", "interior-first"),
                "relaxation": ("none", "chebyshev")}

    def __post_init__(self):
        for name, allowed in self._CHOICES.items():
            if getattr(self, name) not in allowed:
                raise ValueError(f"StencilConfig.{name} must be one of {', '.join(allowed)}; got {getattr(self, name)!r}")
        if self.direct_halo not in (None, True, False, "on", "off", "validate"):
            raise ValueError(f"StencilConfig.direct_halo must be None, a bool, 'on', 'off' or 'validate'; "
                             f"got {self.direct_halo!r}")
        if self.global_width <= 0 or self.global_height <= 0:
            raise ValueError("StencilConfig: the global grid must be non-empty")
        if self.relaxation == "chebyshev":
            if self.kind != "jacobi5":
                raise ValueError("StencilConfig: relaxation='chebyshev' needs kind='jacobi5'")
            if self.periodic:
                raise ValueError("StencilConfig: relaxation='chebyshev' needs periodic=False (fixed edges on all four "
                                 "sides: the periodic operator is singular)")
            if self.init == "rank":
                raise ValueError("StencilConfig: relaxation='chebyshev' does not run the reference's exchange-only init")
        if self.source:
            if self.kind != "jacobi5":
                raise ValueError("StencilConfig: source=True needs kind='jacobi5' (the 5-point Jacobi stencil)")
            if self.periodic:
                raise ValueError("StencilConfig: source=True needs periodic=False (fixed edges on all four sides: the "
                                 "periodic operator is singular)")
            if not self.block_fixed_edges:
                raise ValueError("StencilConfig: source=True needs block_fixed_edges=True (a cycle is one time-blocked "
                                 "pass beside the fixed edges)")
            if self.init == "rank":
                raise ValueError("StencilConfig: source=True does not run the reference's exchange-only init")
            depths = (20, 24) if self.dtype == "f32" else (12, 16)
            if self.time_block > 0 and self.time_block not in depths:
                raise ValueError(f"StencilConfig: source=True needs a time block with level kernels ({self.dtype}: "
                                 f"{depths[0]} or {depths[1]}; 0 picks {depths[1]}), got time_block={self.time_block}")
        if not 0.0 <= self.min_gain < 1.0 or self.wire_delay_us < 0 or self.halo_max_ctas < 0:
            raise ValueError("StencilConfig: min_gain in [0, 1), wire_delay_us >= 0, halo_max_ctas >= 0")

    @property
    def halo(self) -> int:
        if self.kind == "box":
            k = int(round(math.sqrt(len(self.box_weights)))) if self.box_weights else 3
            return max(self.stencil_width // 2, (k - 1) // 2)
        return max(1, self.stencil_width // 2)


class Stencil2D:
    def __init__(self, cfg: StencilConfig, ctx: DistContext | None = None, device: str | None = None):
        self.cfg = cfg
        self.ctx = ctx or DistContext()
        dev = torch.device(device) if device else self.ctx.device
        self.device = dev
        rows, cols = choose_dims(self.ctx.world_size, cfg.dims, cfg.prefer)
        self.decomp = Decomposition(cfg.global_width, cfg.global_height, rows, cols, self.ctx.rank,
                                    (cfg.periodic, cfg.periodic))
        d = self.decomp
        self.dtype = _DTYPES[cfg.dtype]
        h = cfg.halo
        # Temporal blocking only for the GPU Jacobi solver and not for the reference's
        # exchange-only run (its dumps show a stencil_width/2 ghost ring).
        # A ghost ring deeper than a neighbour's tile would need cells two tiles away.
        tb = cfg.time_block
        # A relaxation cycle is one time block: the deeper level kernels' depth
        # unless it exceeds the tile (the native solver's rule).
        self.relaxation = cfg.relaxation == "chebyshev"
        self.source = bool(cfg.source)  # a source's cycles are level-table cycles too (a uniform table)
        self._g_core = None  # torch backend: this rank's slice of g and the cycle's correction G
        self._G = None
        if (self.relaxation or self.source) and tb <= 0 and dev.type == "cuda":
            big, small = (24, 20) if cfg.dtype == "f32" else (16, 12)
            tb = int(self.ctx.allreduce_min(big if big <= min(d.width, d.height) else small))
        # A fast form may run: the sum form (equal coefficients) or the scaled
        # form (unequal, c_neighbor != 0); both take the same time blocks.
        self.sum_form = bool(cfg.sum_form and (cfg.c_center == cfg.c_neighbor or cfg.c_neighbor != 0.0))
        if tb <= 0 and dev.type == "cuda":
            tb = hip().auto_time_block(d.width, d.height, cfg.dtype, self.sum_form)
            # The time block sets the ghost depth and the exchanges per call: the
            # same on every rank (an uneven decomposition gives ranks different
            # tile sizes, and the per-tile default could differ).
            tb = int(self.ctx.allreduce_min(tb))
        # A physical (non-periodic) edge holds fixed boundary values that the
        # S-step kernels would advance as cells: time blocking needs every edge
        # to be a neighbour's, or block_fixed_edges (the frame along the fixed
        # edges on the held-side kernel); the native solver enforces the same rule.
        self.time_block = (max(1, min(tb, d.width, d.height))
                           if (dev.type == "cuda" and cfg.kind == "jacobi5" and cfg.init != "rank"
                               and (cfg.periodic or cfg.block_fixed_edges)) else 1)
        h = max(h, self.time_block)
        C = core()
        if dev.type == "cuda":
            self.geom = C.TileGeom.aligned(d.width, d.height, h, h, self.dtype.itemsize)
        else:
            self.geom = C.TileGeom.compact(d.width, d.height, h, h)
        n = self.geom.alloc_elems()
        self.a = torch.empty(n, dtype=self.dtype, device=dev)
        self.b = torch.empty(n, dtype=self.dtype, device=dev)
        self._init_data()
        self.iteration = 0  # Jacobi iterations applied to the field (checkpoint header)

        # Ranks on this rank's GPU (device UUIDs compared over all ranks, not
        # counts: a launcher that gives each rank one visible device makes every
        # rank see "1 device" on distinct GPUs, and RCCL is then the backend).
        self.gpu_sharing = gpu_sharing(self.ctx, dev)
        self.shared_gpu = self.gpu_sharing > 1
        backend = cfg.backend
        if dev.type != "cuda":
            backend = "torch"
        elif backend == "auto":
            if self.ctx.world_size == 1:
                backend = "rccl" if cfg.loopback else "local"
            else:
                # RCCL refuses two ranks on one GPU: ranks sharing GPUs use the IPC backend.
                backend = "ipc" if self.shared_gpu else "rccl"
        # overlap=None (auto): only for one-exchange-per-iteration runs (S = 1).
        # With temporal blocking the exchange is ~5-8% of a super-step and the
        # concurrent thin boundary strips cost more than they hide (docs/PERF.md,
        # "Multi-GPU schedule"); ranks sharing a GPU never overlap (their
        # cross-process waits + a forked branch oversubscribe the GPU queues).
        auto_overlap = self.time_block == 1 and not self.shared_gpu
        overlap = auto_overlap if cfg.overlap is None else bool(cfg.overlap)
        self.backend = backend
        self.comm = None
        self.solver = None
        self._cur, self._nxt = self.a, self.b
        if backend in ("rccl", "local", "ipc"):
            H = hip()
            # Ranks sharing this GPU: each persistent kernel takes its share of
            # the chip, so all of them are resident at once.
            H.set_gpu_share(self.gpu_sharing)
            if backend == "rccl":
                self.comm = self.ctx.native_comm()
            torch.cuda.synchronize()
            kind = H.StencilKind.BOX if cfg.kind == "box" else H.StencilKind.JACOBI5
            be = {"rccl": H.HaloBackend.RCCL, "local": H.HaloBackend.LOCAL, "ipc": H.HaloBackend.IPC}[backend]
            # Host allgather (through the rendezvous store): the IPC backend's
            # set-up and every collective agreement of the solver (time block,
            # opening, sum-form range, direct-halo validation) — the same path
            # whatever the backend, so the one-GPU multi-rank tests run the code
            # an N-GPU RCCL run agrees with.
            boot = None
            if backend == "ipc" or self.ctx.world_size > 1:
                def boot(blob: bytes, _ctx=self.ctx, _H=H) -> list[bytes]:
                    return _ctx.allgather_bytes(blob, timeout_s=_H.comm_timeout() or None)
            weights = [float(w) for w in cfg.box_weights] if cfg.kind == "box" else []
            radius = (int(round(math.sqrt(len(weights)))) - 1) // 2 if weights else 1
            self.solver = H.StencilSolver(d.topo, d.rank, self.geom, self.a.data_ptr(), self.b.data_ptr(), self.comm,
                                          cfg.dtype, be, overlap, cfg.graph, cfg.loopback, kind, cfg.c_center,
                                          cfg.c_neighbor, radius, weights, cfg.variant, cfg.fuse_periodic,
                                          self.time_block, boot, cfg.graph_supersteps, self.sum_form,
                                          self._direct_mode(backend),
                                          cfg.graph_max_superstep_us, cfg.opening, cfg.rehearse_peers, cfg.min_gain,
                                          cfg.halo_max_ctas, cfg.main_priority, cfg.side_priority,
                                          cfg.wire_delay_us, cfg.direct_engine, cfg.steady,
                                          block_fixed_edges=bool(cfg.block_fixed_edges and not cfg.periodic),
                                          relaxation=cfg.relaxation, global_width=cfg.global_width,
                                          global_height=cfg.global_height, source=self.source)
            # The solver may cap the request (blocks > 16 need the fp32 pipeline's
            # preconditions); the ghost ring was sized for the request.
            self.time_block = self.solver.time_block()
            self.cycle = int(self.solver.relaxation_info()["cycle"])
        else:
            self.plan = make_plan(d, self.geom, corners=True)
            self.halo = TorchHalo(self.plan, self.ctx)
            self.cycle = 0
            if self.relaxation or self.source:
                self.cycle = cfg.time_block if cfg.time_block > 1 else (24 if cfg.dtype == "f32" else 16)
                # A source without Chebyshev: the uniform table, every level the base pair.
                self._levels = ([cfg.c_center] * self.cycle, [cfg.c_neighbor] * self.cycle, 1.0)
            if self.relaxation:
                # The same schedule one iteration at a time: iteration t runs
                # level t mod M through ops.stencil5. The table is the native
                # function's, rank 0's bits on every rank.
                import struct

                t = C.chebyshev_cycle(cfg.global_width, cfg.global_height, cfg.c_center, cfg.c_neighbor, self.cycle)
                blob = struct.pack(f"<{2 * self.cycle + 1}d", *t["center"], *t["neighbor"], t["growth"])
                v = struct.unpack(f"<{2 * self.cycle + 1}d", self.ctx.allgather_bytes(blob)[0])
                self._levels = (list(v[:self.cycle]), list(v[self.cycle:2 * self.cycle]), v[-1])

    # ---------------------------------------------------------------- setup
    def _direct_mode(self, backend: str) -> str:
        """SolverConfig direct halo: "on" for IPC (default), "validate" where asked
        (RCCL or IPC: prepare() checks it bitwise against the backend and times it),
        else "off"."""
        d = self.cfg.direct_halo
        if d == "validate":
            return "validate" if backend in ("rccl", "ipc") and self.ctx.world_size > 1 else "off"
        if backend == "ipc" and d is not False and d != "off":
            return "on"
        return "off"

    def _init_data(self):
        d, g = self.decomp, self.geom
        if self.cfg.init == "rank":
            # Reference: whole tile -1, core = rank id (mpi-2d-stencil-subarray.cpp:77-88).
            ops.fill(self.a, -1.0)
            ops.fill_region(self.a, g.core(), float(d.rank))
            ops.fill(self.b, -1.0)
        else:
            ops.fill(self.a, 0.0)
            ops.fill(self.b, 0.0)
            ops.fill_random(self.a, g, d.x0, d.y0, d.global_width, self.cfg.seed)

    def set_boundary(self, top=None, bottom=None, left=None, right=None):
        """Fixed boundary values of a non-periodic grid: each argument is a scalar
        or a 1-D tensor over the GLOBAL width (top, bottom) or height (left,
        right); None leaves that side as it is. Collective in spirit (every rank
        calls it with the same values), no communication.

        Every rank writes its slice into the ghost row / column adjacent to its
        core on its physical sides, in both buffers (no exchange ever writes a
        physical side, and a pass reads the ring of whichever buffer is
        current). The slice includes the part beside a neighbour's ghost columns
        / rows, clipped to the global range: a rank with a physical top and a
        left neighbour holds row -1 over its left ghost columns too, and nobody
        exchanges those cells (that diagonal has no rank), so boundary values
        must come from this call or from the uniform initial ring. The four
        outside corners are never read by a 5-point stencil. Ends with
        field_changed()."""
        d, g = self.decomp, self.geom
        if self.cfg.periodic:
            raise ValueError("set_boundary: the grid is periodic (StencilConfig.periodic=False has fixed edges)")
        null = core().PROC_NULL
        hx, hy = g.halo_x, g.halo_y
        # Global index range of the ring row / column next to this tile, clipped.
        gx_lo, gx_hi = max(0, d.x0 - hx), min(d.global_width, d.x0 + d.width + hx)
        gy_lo, gy_hi = max(0, d.y0 - hy), min(d.global_height, d.y0 + d.height + hy)

        def values(v, n, lo, hi, what):
            if isinstance(v, torch.Tensor):
                if v.dim() != 1 or v.numel() != n:
                    raise ValueError(f"set_boundary: {what} must be a scalar or a 1-D tensor of {n} values")
                return v[lo:hi].to(device=self.device, dtype=self.dtype)
            return torch.full((hi - lo,), float(v), device=self.device, dtype=self.dtype)

        self.synchronize()
        for buf in (self.a, self.b):
            full = buf.view(g.total_height(), g.pitch)[:, g.x_origin:g.x_origin + g.total_width()]
            cols = slice(hx + gx_lo - d.x0, hx + gx_hi - d.x0)
            rows = slice(hy + gy_lo - d.y0, hy + gy_hi - d.y0)
            if top is not None and d.topo.shift(d.rank, 0, -1) == null:
                full[hy - 1, cols] = values(top, d.global_width, gx_lo, gx_hi, "top")
            if bottom is not None and d.topo.shift(d.rank, 0, 1) == null:
                full[hy + g.height, cols] = values(bottom, d.global_width, gx_lo, gx_hi, "bottom")
            if left is not None and d.topo.shift(d.rank, -1, 0) == null:
                full[rows, hx - 1] = values(left, d.global_height, gy_lo, gy_hi, "left")
            if right is not None and d.topo.shift(d.rank, 1, 0) == null:
                full[rows, hx + g.width] = values(right, d.global_height, gy_lo, gy_hi, "right")
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        self.field_changed()

    def fixed_edge_note(self) -> str:
        """Time blocking beside fixed edges: this rank's held sides and its
        interior / frame split ('' when inactive)."""
        return self.solver.fixed_edge_note() if self.solver is not None else ""

    # ------------------------------------------------------------- stepping
    def step(self):
        self.run(1)

    def run(self, iters: int):
        if iters <= 0:
            return
        if self.cycle and iters % self.cycle:
            mode = "relaxation='chebyshev'" if self.relaxation else "source=True"
            raise ValueError(f"run({iters}): with {mode} the cycle is the unit of progress, so the "
                             f"iteration count must be a multiple of the cycle length {self.cycle}")
        if self.solver is not None:
            self.solver.run(iters)
            self.iteration += iters
            return
        self._last_iters = iters
        for _ in range(iters):
            self._python_step()
            self.iteration += 1

    def prepare(self, iters: int):
        """Collective: take every one-off cost of a later ``run(iters)`` now
        (graph capture + upload, first launch of each kernel shape) without
        advancing the field. Benchmarks call it before their timed window."""
        if self.solver is not None and iters > 0:
            self.solver.prepare(iters)

    def warm(self, iters: int, seconds: float, tail: int = 0) -> int:
        """Collective: about ``seconds`` of untimed, state-preserving passes of
        ``run(iters)``'s kernel shapes, so a short timed window that follows runs
        at the device's sustained clocks instead of paying the DVFS ramp (a cold
        20-step window at 32768^2 is ~20% slower than a warm one). The pass count
        is agreed across ranks (max of the per-rank estimates). ``tail``: that
        many more single passes after the burst has drained, each drained too, so
        the window that follows is the next of back-to-back windows rather than
        the first after the burst. Returns the passes run."""
        if self.solver is None or iters <= 0 or seconds <= 0:
            return 0
        self.solver.synchronize()
        t0 = time.perf_counter()
        self.solver.warm(iters, 1)
        one = max(time.perf_counter() - t0, 1e-5)
        passes = int(self.ctx.allreduce_max(min(1000.0, math.ceil(seconds / one))))
        self.solver.warm(iters, passes)
        for _ in range(max(0, tail)):
            self.solver.warm(iters, 1)
        return passes + 1 + max(0, tail)

    def _python_step(self):
        cfg, g = self.cfg, self.geom
        self.halo.exchange(self._cur)
        if cfg.kind == "box":
            ops.stencil_box(self._cur, self._nxt, g, 0, g.width, 0, g.height, cfg.box_weights)
        elif self.cycle:  # level t mod M of the cycle
            lvl = self.iteration % self.cycle
            ops.stencil5(self._cur, self._nxt, g, 0, g.height, self._levels[0][lvl], self._levels[1][lvl])
            if self._G is not None and lvl == self.cycle - 1:  # the cycle's correction, one rounded add per cell
                out = self._core_of(self._nxt)
                out.copy_(out + self._G)
        else:
            ops.stencil5(self._cur, self._nxt, g, 0, g.height, cfg.c_center, cfg.c_neighbor)
        self._cur, self._nxt = self._nxt, self._cur

    def _core_of(self, tile: torch.Tensor) -> torch.Tensor:
        g = self.geom
        x0 = g.x_origin + g.halo_x
        return tile.view(g.total_height(), g.pitch)[g.halo_y:g.halo_y + g.height, x0:x0 + g.width]

    def set_source(self, g):
        """Collective: the source term ``g`` of ``u' = A u + g`` (``StencilConfig.source``):
        a scalar, a 2-D tensor over the GLOBAL grid (``global_height x global_width``,
        any device; each rank takes its core's slice) or ``None``, which clears the
        source. ``g`` is the additive term of one base Jacobi step; for
        ``-laplace(u) = f`` with the 5-point average it is ``c_neighbor h^2 f``.

        Builds the cycle's correction ``G`` (``G_0 = 0``, ``G_{l+1} = C_l G_l + w_l g``:
        one single step and one halo exchange per level, on a tile whose ring is 0
        on physical sides), which every later cycle adds where it stores;
        ``residual()`` becomes ``A u + g - u``. Drops captured graphs and ends like
        ``field_changed()``. Until it is called the solver runs the homogeneous
        level passes. The source is not part of a checkpoint: call it again
        after ``load_checkpoint``."""
        if not self.source:
            raise ValueError("set_source: this solver was built without a source term (StencilConfig.source=True)")
        d, geom = self.decomp, self.geom
        tile = None
        if g is not None:
            tile = torch.zeros(geom.alloc_elems(), dtype=self.dtype, device=self.device)
            if isinstance(g, torch.Tensor):
                if g.dim() != 2 or tuple(g.shape) != (d.global_height, d.global_width):
                    raise ValueError(f"set_source: g must be a scalar or a 2-D tensor of shape (global_height, "
                                     f"global_width) = ({d.global_height}, {d.global_width}); got {tuple(g.shape)}")
                mine = g[d.y0:d.y0 + d.height, d.x0:d.x0 + d.width].to(device=self.device, dtype=self.dtype)
            else:
                mine = torch.full((d.height, d.width), float(g), dtype=self.dtype, device=self.device)
            self._core_of(tile).copy_(mine)
        self.synchronize()
        if self.solver is not None:
            if self.device.type == "cuda":
                torch.cuda.synchronize()
            self.solver.set_source(tile.data_ptr() if tile is not None else 0)  # the solver keeps its own copies
            return
        self._g_core, self._G = None, None
        if tile is not None:
            from ..ops.source import level_omega

            g_core = self._core_of(tile).clone()
            a, b = torch.zeros_like(tile), torch.zeros_like(tile)
            for c0, c1 in zip(self._levels[0], self._levels[1]):
                self.halo.exchange(a)
                ops.stencil5(a, b, geom, 0, geom.height, c0, c1)
                p = torch.tensor(level_omega(c1, self.cfg.c_neighbor), dtype=self.dtype, device=self.device) * g_core
                out = self._core_of(b)
                out.copy_(out + p)
                a, b = b, a
            G = self._core_of(a).clone()
            finite = bool(torch.isfinite(G).all())
            if self.ctx.allreduce_max(0.0 if finite else 1.0) != 0.0:
                raise RuntimeError("set_source: the cycle's correction G is not finite (the source or the level table "
                                   "overflows the element type)")
            self._g_core, self._G = g_core, G
        self.field_changed()

    def source_correction(self) -> torch.Tensor | None:
        """This rank's core of the cycle's correction ``G`` (a copy; ``None`` while
        no source is set)."""
        if self.solver is None:
            return None if self._G is None else self._G.clone()
        flat = torch.empty(self.geom.alloc_elems(), dtype=self.dtype, device=self.device)
        torch.cuda.synchronize()
        if not self.solver.copy_source_correction(flat.data_ptr()):
            return None
        return self._core_of(flat).clone()

    def relaxation_note(self) -> str:
        """The relaxation cycle: which passes run and why (the level passes, or the
        plain per-step pass when the range guard growth x max|u| < max(T) / 4
        fails), with M, the weights' range and the prefix growth ('' for plain
        Jacobi)."""
        if self.solver is not None:
            return self.solver.relaxation_note()
        if not self.cycle:
            return ""
        info = self.relaxation_info()
        if not self.relaxation:
            return (f"uniform level table (source=True): M = {self.cycle}; one level per iteration through "
                    "ops.stencil5 (the field is the iterate at cycle ends only)")
        return (f"chebyshev: M = {self.cycle}, omega in [{info['omega_min']:.4g}, {info['omega_max']:.4g}], "
                f"growth {info['growth']:.4g}; one level per iteration through ops.stencil5 (the field is meaningful "
                "at cycle ends only)")

    def relaxation_info(self) -> dict:
        """``{"cycle", "omega_min", "omega_max", "growth"}`` of the agreed cycle
        (cycle 0 for plain Jacobi)."""
        if self.solver is not None:
            i = self.solver.relaxation_info()
            return {k: i[k] for k in ("cycle", "omega_min", "omega_max", "growth")}
        if not self.cycle:
            return {"cycle": 0, "omega_min": 0.0, "omega_max": 0.0, "growth": 0.0}
        omega = [1.0 if n == self.cfg.c_neighbor else n / self.cfg.c_neighbor for n in self._levels[1]]
        return {"cycle": self.cycle, "omega_min": min(omega), "omega_max": max(omega), "growth": self._levels[2]}

    # ---------------------------------------------------------- convergence
    MAX_RESIDUAL_HISTORY = 4096  # checks kept in run_until()'s history (StencilSolver: kMaxResidualHistory)
    # run_until's default chunk in time blocks (StencilSolver: kDefaultCheckBlocks; measured, docs/PERF.md).
    DEFAULT_CHECK_BLOCKS = 16

    def residual(self) -> dict:
        """Collective (jacobi5): the norms of the Jacobi residual ``r = A u - u``
        (``A u + g - u`` once ``set_source`` set a source)
        over the global core — exactly the change the next single step would
        make — agreed over ranks: ``{"linf": max |r|, "l2": sqrt(sum r^2),
        "cells": global cells}``. It needs the current field and a fresh 1-deep
        ghost ring only (beside a fixed edge the ring holds the boundary
        values), and leaves the field unchanged. The native solver runs the HIP
        kernel ``ops.stencil5_residual``; the torch backend exchanges through
        ``TorchHalo`` and evaluates the reference expression."""
        if self.cfg.kind != "jacobi5":
            raise ValueError("residual: only the 5-point Jacobi stencil has a residual (kind is 'box')")
        if self.solver is not None:
            r = self.solver.residual()
            return {"linf": float(r["linf"]), "l2": float(r["l2"]), "cells": int(r["cells"])}
        g = self.geom
        self.halo.exchange(self._cur)
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        v = self._cur.view(g.total_height(), g.pitch)[:, g.x_origin:g.x_origin + g.total_width()]
        linf, l2 = ops.residual5_reference(v, (g.halo_y, g.halo_x), self.cfg.c_center, self.cfg.c_neighbor,
                                           source=self._g_core)
        # A NaN travels as +inf (a max of NaNs depends on the order); the squares
        # are summed in rank order, so every rank gets the same bits.
        linf = self.ctx.allreduce_max(linf if math.isfinite(linf) else math.inf)
        sumsq = sum(self.ctx.gather_floats(l2 * l2)) if self.ctx.is_distributed else l2 * l2
        return {"linf": linf, "l2": math.sqrt(sumsq) if sumsq >= 0 else math.nan, "cells": self.cells_per_step}

    def run_until(self, tol: float, max_iters: int, check_every: int = 0, norm: str = "linf") -> dict:
        """Collective: iterate until converged. Checks the residual first (an
        already converged field returns after 0 iterations), then repeats
        ``run(min(check_every, remaining))`` + ``residual()`` until the agreed
        norm (``"linf"`` or ``"l2"``) is <= ``tol``, ``max_iters`` iterations
        ran, or the norm is not finite (stops at once). ``check_every=0``:
        ``DEFAULT_CHECK_BLOCKS`` (16) x the time block. Every rank stops at the same iteration. Returns
        ``{"converged", "iterations", "residual", "checks", "reason", "norm",
        "history": [(iteration, linf, l2), ...]}``; ``self.iteration`` advances
        by the iterations actually run. With relaxation='chebyshev'
        ``check_every`` is rounded up and ``max_iters`` down to whole cycles;
        the result's ``"check_every"`` and ``"max_iters"`` are the values used."""
        if self.cfg.kind != "jacobi5":
            raise ValueError("run_until: only the 5-point Jacobi stencil has a residual (kind is 'box')")
        if norm not in ("linf", "l2"):
            raise ValueError(f"run_until: norm must be 'linf' or 'l2', got {norm!r}")
        if not tol >= 0:
            raise ValueError(f"run_until: tol must be >= 0, got {tol}")
        if max_iters < 0 or check_every < 0:
            raise ValueError(f"run_until: max_iters and check_every must be >= 0, got {max_iters}, {check_every}")
        if self.solver is not None:
            out = dict(self.solver.run_until(float(tol), int(max_iters), int(check_every), norm))
            out["history"] = [tuple(h) for h in out["history"]]
            self.iteration += out["iterations"]
            return out
        every = check_every if check_every > 0 else self.DEFAULT_CHECK_BLOCKS * max(self.time_block, self.cycle)
        if self.cycle:  # whole cycles: the chunk up, the cap down
            every = -(-every // self.cycle) * self.cycle
            max_iters = max_iters // self.cycle * self.cycle
        out = {"converged": False, "iterations": 0, "residual": 0.0, "checks": 0, "check_every": every,
               "max_iters": max_iters, "reason": "", "norm": norm, "history": []}
        while True:
            r = self.residual()
            out["checks"] += 1
            out["residual"] = r[norm]
            if len(out["history"]) < self.MAX_RESIDUAL_HISTORY:
                out["history"].append((out["iterations"], r["linf"], r["l2"]))
            if not (math.isfinite(r[norm]) and math.isfinite(r["linf"])):
                out["reason"] = "non-finite residual"
                break
            if r[norm] <= tol:
                out["converged"] = True
                out["reason"] = f"converged: {norm} residual <= tol"
                break
            if out["iterations"] >= max_iters:
                out["reason"] = "max_iters reached"
                break
            n = min(every, max_iters - out["iterations"])
            self.run(n)
            out["iterations"] += n
        return out

    def exchange(self):
        """One halo exchange of the current tile, no update (the reference's run)."""
        if self.solver is not None:
            self.solver.exchange_only()
            self.solver.synchronize()
        else:
            self.halo.exchange(self._cur)

    def synchronize(self):
        if self.solver is not None:
            self.solver.synchronize()
        elif self.device.type == "cuda":
            torch.cuda.synchronize()

    def watchdog(self, timeout_s: float, what: str = "stencil halo exchange (RCCL)"):
        """A deadline for a blocking wait outside the solver (``torch.cuda.synchronize()``
        on the solver's work): past it the RCCL communicators the halo uses are
        aborted and leaving the block raises (parallel/watchdog.py)."""
        from ..parallel.watchdog import CommWatchdog

        aborts = []
        if self.solver is not None and self.comm is not None:
            aborts = [self.solver.abort_halo_comm, self.comm.abort]
        return CommWatchdog(timeout_s, aborts, what)

    # ---------------------------------------------------------------- state
    def current(self) -> torch.Tensor:
        """The tensor holding the current field. The caller may write it, so the
        native solver re-exchanges the ghost ring and re-checks the sum form's
        range before its next pass (one extra exchange; see field_changed())."""
        if self.solver is not None:
            self.solver.field_changed()
            return self.a if self.solver.current() == self.a.data_ptr() else self.b
        return self._cur

    def field_changed(self):
        """Tell the native solver that the field was written from outside."""
        if self.solver is not None:
            self.solver.field_changed()

    @property
    def sum_form_active(self) -> bool:
        """Whether the passes run a fast form right now — the sum form (equal
        coefficients) or the scaled form (unequal) — because the coefficients,
        the user's choice and the measured field range all allow it."""
        if self.solver is not None:
            return bool(self.solver.sum_form_active())
        return False

    @property
    def scaled_form_active(self) -> bool:
        """Whether the fast form running is the scaled one (c_center != c_neighbor)."""
        if self.solver is not None:
            return bool(self.solver.scaled_form_active())
        return False

    def last_run_blocks(self) -> list[tuple[int, int]]:
        """(S, count) of the super-steps the last run() executed."""
        if self.solver is not None:
            return [tuple(x) for x in self.solver.last_run_blocks()]
        return [(1, getattr(self, "_last_iters", 0))]  # the torch path: one exchange + one step per iteration

    def full_view(self) -> torch.Tensor:
        """(total_height, total_width) logical view: core + ghost ring."""
        g = self.geom
        v = self.current().view(g.total_height(), g.pitch)
        return v[:, g.x_origin:g.x_origin + g.total_width()]

    def core_view(self) -> torch.Tensor:
        g = self.geom
        return self.full_view()[g.halo_y:g.halo_y + g.height, g.halo_x:g.halo_x + g.width]

    def gather_global(self) -> torch.Tensor | None:
        """Assemble the global core grid on every rank (tests / validation)."""
        import torch.distributed as dist

        self.synchronize()  # the native solver writes on its own streams
        local = self.core_view().detach().cpu().clone()
        d = self.decomp
        if not self.ctx.is_distributed:
            return local
        parts = [None] * self.ctx.world_size
        dist.all_gather_object(parts, (d.x0, d.y0, local))
        out = torch.empty(d.global_height, d.global_width, dtype=local.dtype)
        for x0, y0, t in parts:
            out[y0:y0 + t.shape[0], x0:x0 + t.shape[1]] = t
        return out

    def save_checkpoint(self, path: str):
        """Collective: write the global field to one decomposition-independent
        grid file (format shared with the C++ apps' --checkpoint)."""
        from ..utils import checkpoint

        return checkpoint.save(self, path)

    def load_checkpoint(self, path: str):
        """Collective: resume from a grid file written by any decomposition."""
        from ..utils import checkpoint

        return checkpoint.load(self, path)

    @property
    def cells_per_step(self) -> int:
        return self.cfg.global_width * self.cfg.global_height

    def graph_status(self) -> str:
        return self.solver.graph_status() if self.solver is not None else "python loop"

    def halo_mode(self) -> str:
        """How the last run() refreshed the halo: what it executed (its super-steps,
        their exchanges and the opening), not what the solver could do."""
        if self.solver is None:
            return "torch-p2p (one exchange per iteration)"
        blocks = self.last_run_blocks()
        steps = sum(s * n for s, n in blocks)
        passes = sum(n for _, n in blocks)
        if not passes:
            return "no run yet"
        shape = " + ".join(f"{n} x {s}-step" for s, n in blocks if n)
        what = f"{steps} iterations as {shape} pass{'es' if passes > 1 else ''}"
        if self.solver.fused_periodic():
            return f"{what}; no exchange (1x1 periodic: the self-halo is the kernel's wrap-around addressing)"
        ex = self.solver.last_run_exchanges()
        opening = self.solver.last_run_opening()
        how = {"rccl": "RCCL send/recv per peer (pack -> ncclSend/ncclRecv -> unpack)",
               "ipc": "HIP IPC", "local": "local self-copy"}.get(self.backend, self.backend)
        if self.solver.direct_halo():
            how = ("HIP IPC direct push of each pass's edge bands into the neighbours' tiles"
                   + (" by the SDMA copy engines" if self.cfg.direct_engine == "copy-engine" else ""))
        text = f"{what}; {ex} halo exchange{'s' if ex != 1 else ''} by {how}"
        if self.solver.fixed_edge_note():
            text += f"; fixed edges: {self.solver.fixed_edge_note()}"
        wd = self.solver.wire_delay_us()
        if wd:
            text += f" (+ {wd:g} us of rehearsed wire time after each transfer)"
        steady = self.solver.schedule_times().get("steady") == "interior-first"
        if opening == "interior-first" and steady and passes > 1:
            text += ("; every super-step interior-first (its exchange ran under the chunks that read only core "
                     "cells, the ghost-ring chunks after it)")
        elif opening == "interior-first":
            text += ("; opening interior-first (the priming exchange ran under the chunks that read only core "
                     "cells, the ghost-ring chunks after it)")
        elif opening == "serial":
            text += "; opening serial (priming exchange, then the pass)"
        elif opening == "overlap":
            text += "; thin-strip overlap (interior on a second stream while each exchange runs)"
        if (self.solver.multi_rank() and not self.solver.direct_halo() and not self.solver.overlapped()
                and not (steady and opening == "interior-first")):
            text += "; the call's last pass is bare (the next call primes)"
        return text

    def profile_window(self, iters: int) -> dict:
        """Collective, state-preserving: one event-timed replica of ``run(iters)``'s
        opening super-step (host enqueue, pack / RCCL / unpack, passes, tail)."""
        if self.solver is None:
            return {}
        p = self.solver.profile_window(iters)
        return {"opening": p["opening"], "exchanges": p["exchanges"],
                "host_enqueue_us": round(p["host_enqueue_us"], 1), "gpu_span_us": round(p["gpu_span_us"], 1),
                "wall_us": round(p["wall_us"], 1),
                "host_overhead_us": round(p["wall_us"] - p["gpu_span_us"], 1),
                # The same replica without phase events: its wall time over the GPU span.
                "plain_wall_us": round(p["plain_wall_us"], 1),
                "plain_wall_over_span": round(p["plain_wall_us"] / p["gpu_span_us"], 3) if p["gpu_span_us"] else None,
                "phases_us": {name: [round(t0, 1), round(t1, 1)] for name, t0, t1 in p["phases"]}}

    # ----------------------------------------------------------------- dump
    def dump_text(self, stage_arrays: list[tuple[str, torch.Tensor]], device_id: int | None = None,
                  stencil=(None, None)) -> str:
        """Per-rank file text in the reference format (stencil2d/sample-output/*)."""
        d = self.decomp
        sw = stencil[0] or self.cfg.stencil_width
        sh = stencil[1] or self.cfg.stencil_width
        lines = [f"Rank:  {d.rank}", f"Coord: {d.row}, {d.col}"]
        if device_id is not None:
            lines += ["", f"HIP device id: {device_id}"]
        lines += ["", "Compute grid"]
        text = "\n".join(lines) + "\n" + d.topo.grid_text() + "\n"
        text += f"{d.width} x {d.height} grid size\n"
        text += f"{d.width + 2 * (sw // 2)} x {d.height + 2 * (sh // 2)} total(with ghost/halo regions) grid size\n"
        text += f"{sw} x {sh} stencil\n\n"
        for i, (title, arr) in enumerate(stage_arrays):
            text += title + "\n" + format_tile(arr)
            if i + 1 < len(stage_arrays):
                text += "\n"
        return text


def gpu_sharing(ctx: DistContext, dev: torch.device) -> int:
    """How many ranks of ``ctx`` run on ``dev``'s GPU (this one included), by
    device UUID (collective when distributed)."""
    if dev.type != "cuda":
        return 1
    props = torch.cuda.get_device_properties(dev)
    ident = str(getattr(props, "uuid", "") or getattr(props, "pci_bus_id", "") or dev.index).encode()
    if not ctx.is_distributed:
        return 1
    return sum(1 for other in ctx.allgather_bytes(ident) if other == ident)


def format_tile(arr: torch.Tensor) -> str:
    """Rows of space-terminated values, std::ostream-default (%g) formatting."""
    a = arr.detach().cpu().double().tolist()
    return "".join("".join(f"{v:g} " for v in row) + "\n" for row in a)


# --------------------------------------------------------------------- CLI
def _parse_wh(s: str) -> tuple[int, int]:
    w, h = s.lower().split("x")
    return int(w), int(h)


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="2D domain-decomposed stencil (MI355X-native)")
    p.add_argument("--global", dest="global_", default=None, help="global grid WxH (default 8192x8192)")
    p.add_argument("--local", default=None, help="per-rank tile WxH (overrides --global)")
    p.add_argument("--dims", default=None, help="process grid RxC (default: wide MPI_Dims_create)")
    p.add_argument("--dtype", default="f32", choices=list(_DTYPES))
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--backend", default="auto", choices=["auto", "rccl", "ipc", "local", "torch"])
    p.add_argument("--no-overlap", action="store_true")
    p.add_argument("--no-graph", action="store_true")
    p.add_argument("--loopback", action="store_true")
    p.add_argument("--variant", default="auto", choices=["auto", "roll", "lds"])
    p.add_argument("--time-block", type=int, default=StencilConfig.time_block)
    p.add_argument("--opening", default="auto", choices=["auto", "serial", "interior-first"])
    p.add_argument("--steady", default="auto", choices=["auto", "serial", "interior-first"])
    p.add_argument("--c-center", type=float, default=StencilConfig.c_center)
    p.add_argument("--c-neighbor", type=float, default=StencilConfig.c_neighbor)
    p.add_argument("--no-sum-form", action="store_true",
                   help="per-step evaluation (bitwise equal to S single steps) instead of the sum / scaled form")
    p.add_argument("--non-periodic", action="store_true", help="fixed (non-periodic) edges on all four sides")
    p.add_argument("--block-fixed-edges", action="store_true",
                   help="with --non-periodic: keep the time block (interior on the usual kernels, the frame along "
                        "the fixed edges on the held-side kernel) instead of one exchange per iteration")
    p.add_argument("--relaxation", default="none", choices=["none", "chebyshev"],
                   help="chebyshev: each time block is one Chebyshev cycle (needs --non-periodic --block-fixed-edges; "
                        "--iters, --warmup and --check-every in whole cycles; the field is meaningful at cycle ends)")
    p.add_argument("--source", type=float, default=None, metavar="Q",
                   help="a constant source term g = Q everywhere (u' = A u + g); implies --non-periodic and "
                        "--block-fixed-edges and needs a time block with level kernels (fp32 20 / 24, fp64 12 / 16; "
                        "the default picks one); --iters, --warmup and --check-every in whole cycles")
    p.add_argument("--tol", type=float, default=None,
                   help="iterate until the residual norm is <= TOL (run_until) instead of --iters iterations; "
                        "the timed region is the run_until")
    p.add_argument("--max-iters", type=int, default=None, help="with --tol: the iteration cap (default: --iters)")
    p.add_argument("--check-every", type=int, default=0,
                   help="with --tol: iterations between residual checks (0 = 16 x the time block)")
    p.add_argument("--norm", default="linf", choices=["linf", "l2"], help="with --tol: the norm compared with TOL")
    p.add_argument("--seed", type=int, default=StencilConfig.seed)
    p.add_argument("--checkpoint", default=None, help="write the final field to this grid file")
    p.add_argument("--resume", default=None, help="start from this grid file (any decomposition)")
    p.add_argument("--json", default=None)
    args = p.parse_args(argv)
    ctx = dist_init()
    rows, cols = choose_dims(ctx.world_size, args.dims, "wide")
    if args.local:
        lw, lh = _parse_wh(args.local)
        gw, gh = lw * cols, lh * rows
    else:
        gw, gh = _parse_wh(args.global_ or "8192x8192")
    if args.source is not None:  # the source's preconditions come with it
        args.non_periodic = args.block_fixed_edges = True
    cfg = StencilConfig(global_width=gw, global_height=gh, dims=f"{rows}x{cols}", dtype=args.dtype,
                        backend=args.backend, overlap=False if args.no_overlap else None, graph=not args.no_graph,
                        loopback=args.loopback, variant=args.variant, time_block=args.time_block,
                        seed=args.seed, opening=args.opening, steady=args.steady, c_center=args.c_center,
                        c_neighbor=args.c_neighbor, sum_form=not args.no_sum_form, periodic=not args.non_periodic,
                        block_fixed_edges=args.block_fixed_edges, relaxation=args.relaxation,
                        source=args.source is not None)
    st = Stencil2D(cfg, ctx)
    if args.source is not None:
        st.set_source(args.source)
    if args.resume:
        hdr = st.load_checkpoint(args.resume)
        if ctx.is_root:
            print(f"resumed from {args.resume} at iteration {hdr.iteration}", file=sys.stderr)
    st.run(-(-args.warmup // st.cycle) * st.cycle if st.cycle else args.warmup)  # a relaxation cycle: whole cycles
    until = None
    if args.tol is not None:
        cap = args.iters if args.max_iters is None else args.max_iters
        chunk = args.check_every if args.check_every > 0 else Stencil2D.DEFAULT_CHECK_BLOCKS * st.time_block
        if st.cycle:  # run_until's own rounding to whole cycles
            chunk, cap = -(-chunk // st.cycle) * st.cycle, cap // st.cycle * st.cycle
        st.prepare(max(1, min(chunk, cap)))
        st.synchronize()
        ctx.barrier()
        t0 = time.perf_counter()
        until = st.run_until(args.tol, cap, args.check_every, args.norm)
        iters = until["iterations"]
    else:
        st.prepare(args.iters)
        st.synchronize()
        ctx.barrier()
        t0 = time.perf_counter()
        st.run(args.iters)
        iters = args.iters
    st.synchronize()
    ctx.barrier()
    dt = ctx.allreduce_max(time.perf_counter() - t0)
    gcells = st.cells_per_step * iters / dt / 1e9
    rec = {"metric": "stencil2d_gcells_per_s", "value": gcells, "ms_per_iter": dt / max(iters, 1) * 1e3,
           "ranks": ctx.world_size, "dims": f"{rows}x{cols}", "config": asdict(cfg), "backend": st.backend,
           "graph": st.graph_status(), "iteration": st.iteration, "time_block": st.time_block,
           "fixed_edges": st.fixed_edge_note(), "halo_mode": st.halo_mode(),
           "evaluation": ("scaled form" if st.scaled_form_active else "sum form" if st.sum_form_active
                          else "per step")}
    info = st.relaxation_info()
    rec.update(relaxation=cfg.relaxation, cycle=info["cycle"], omega_min=info["omega_min"], omega_max=info["omega_max"],
               cycle_growth=info["growth"], relaxation_note=st.relaxation_note(), source=args.source)
    if until is not None:
        rec.update(converged=until["converged"], iterations=until["iterations"], residual=until["residual"],
                   checks=until["checks"], norm=until["norm"], reason=until["reason"], tol=args.tol,
                   wall_s=dt)
    if args.checkpoint:
        st.save_checkpoint(args.checkpoint)
    if ctx.is_root:
        print(json.dumps(rec))
        if args.json:
            with open(args.json, "a") as f:
                f.write(json.dumps(rec) + "\n")
    ctx.destroy()
    return 0


if __name__ == "__main__":
    sys.exit(main())
