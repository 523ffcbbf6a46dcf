// _mxs_hip: bindings of the HIP kernels and the native runtime (RCCL
// communicator, halo exchanger, stencil solver, ping-pong).
//
// Buffers cross the boundary as raw device addresses (Python ints, e.g.
// torch.Tensor.data_ptr()) and streams as hipStream_t handles
// (torch.cuda.current_stream().cuda_stream), so the Python side keeps using the
// PyTorch caching allocator while all device work is launched from C++.
// Import torch BEFORE this module: then libamdhip64.so.7 / librccl.so.1 resolve
// to the copies torch already loaded (one HIP runtime per process).
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <array>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "mxs/comm/rccl_comm.hpp"
#include "mxs/core/fault.hpp"
#include "mxs/halo/exchange.hpp"
#include "mxs/kernels/kernels.hpp"
#include "mxs/runtime/cg_solver.hpp"
#include "mxs/runtime/ipc.hpp"
#include "mxs/runtime/multigrid_solver.hpp"
#include "mxs/runtime/pcg_solver.hpp"
#include "mxs/runtime/pingpong.hpp"
#include "mxs/runtime/stencil_solver.hpp"

namespace py = pybind11;
using namespace mxs;

namespace {

template <typename T>
T* ptr(std::uintptr_t p) {
  return reinterpret_cast<T*>(p);
}
hipStream_t strm(std::uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

enum class DType { F32, F64 };
DType parse_dtype(const std::string& d) {
  if (d == "f32" || d == "float32" || d == "float") return DType::F32;
  if (d == "f64" || d == "float64" || d == "double") return DType::F64;
  throw std::invalid_argument("unsupported dtype '" + d + "' (use f32 or f64)");
}

// Python callable (bytes -> list[bytes], collective) as the IPC backend's host
// allgather. Only called during construction, with the GIL held.
HostAllgather wrap_allgather(py::object fn) {
  if (fn.is_none()) return {};
  return [fn](const std::string& blob) {
    py::gil_scoped_acquire gil;
    py::list parts = fn(py::bytes(blob));
    std::vector<std::string> out;
    for (auto item : parts) out.push_back(std::string(py::bytes(py::reinterpret_borrow<py::object>(item))));
    return out;
  };
}

kernels::StencilVariant parse_variant(const std::string& v) {
  if (v == "auto") return kernels::StencilVariant::Auto;
  if (v == "roll") return kernels::StencilVariant::RegisterRoll;
  if (v == "lds") return kernels::StencilVariant::LdsTile;
  throw std::invalid_argument("unknown stencil variant '" + v + "' (auto|roll|lds)");
}

// `what`: the argument's name (opening, steady).
Opening parse_opening(const std::string& name, const char* what) {
  if (name == "auto") return Opening::Auto;
  if (name == "serial") return Opening::Serial;
  if (name == "interior-first") return Opening::InteriorFirst;
  throw std::invalid_argument(std::string(what) + " must be auto, serial or interior-first, got '" + name + "'");
}

kernels::DotReduce parse_reduce(const std::string& r) {
  if (r == "atomic") return kernels::DotReduce::Atomic;
  if (r == "two-pass" || r == "two_pass") return kernels::DotReduce::TwoPass;
  if (r == "single-pass" || r == "single_pass" || r == "gpu") return kernels::DotReduce::SinglePass;
  if (r == "host" || r == "cpu") return kernels::DotReduce::HostPartials;
  if (r == "racy" || r == "no-sync") return kernels::DotReduce::Racy;
  throw std::invalid_argument("unknown reduction '" + r + "'");
}

kernels::BoxWeights make_box(int radius, const std::vector<float>& w) {
  kernels::BoxWeights b;
  b.radius = radius;
  const size_t k = size_t(2 * radius + 1) * size_t(2 * radius + 1);
  if (radius < 1 || radius > kernels::kMaxBoxRadius) throw std::invalid_argument("box radius must be 1 or 2");
  if (w.size() != k) throw std::invalid_argument("box weights must have (2r+1)^2 entries");
  for (size_t i = 0; i < k; ++i) b.w[i] = w[i];
  return b;
}

// Type-erased solver handle so Python sees one class per solver.
template <template <class> class Solver>
struct TypedHandle {
  DType dt;
  std::unique_ptr<Solver<float>> f;
  std::unique_ptr<Solver<double>> d;
  template <typename F>
  auto visit(F&& fn) {
    return dt == DType::F32 ? fn(*f) : fn(*d);
  }
  // The solver of `dtype` from its config struct.
  template <typename Config>
  static std::unique_ptr<TypedHandle> make(const std::string& dtype, const Config& cfg) {
    auto h = std::make_unique<TypedHandle>();
    h->dt = parse_dtype(dtype);
    if (h->dt == DType::F32) h->f = std::make_unique<Solver<float>>(cfg);
    else h->d = std::make_unique<Solver<double>>(cfg);
    return h;
  }
};
using SolverHandle = TypedHandle<StencilSolver>;
using MultigridHandle = TypedHandle<MultigridSolver>;
using CgHandle = TypedHandle<CgSolver>;
using PcgHandle = TypedHandle<PcgSolver>;

// Ghost codes (top, bottom, left, right) from Python; set reflect flags turn a far code of 0 into -1.
kernels::GhostSides ghost_sides(const std::array<int, 4>& c, bool reflect_rows = false, bool reflect_cols = false) {
  kernels::GhostSides sd{c[0], c[1], c[2], c[3]};
  if (reflect_rows && sd.bottom == kernels::kGhostRing) sd.bottom = kernels::kGhostReflect;
  if (reflect_cols && sd.right == kernels::kGhostRing) sd.right = kernels::kGhostReflect;
  return sd;
}
const std::array<int, 4> kNoSides{0, 0, 0, 0};

// CgScalars or PcgScalars ("rz" is the latter's alone).
template <typename S>
py::dict scalars_dict(const S& s) {
  py::dict d;
  d["rr"] = s.rr;
  if constexpr (std::is_same<S, kernels::PcgScalars>::value) d["rz"] = s.rz;
  d["pq"] = s.pq;
  d["alpha"] = s.alpha;
  d["beta"] = s.beta;
  d["linf"] = s.linf;
  d["tol"] = s.tol;
  d["iteration"] = s.iteration;
  d["max_iters"] = s.max_iters;
  d["norm"] = s.norm;
  d["status"] = s.status;
  return d;
}

// CgResidual or MultigridResidual.
template <typename R>
py::dict residual_dict(const R& r) {
  py::dict d;
  d["linf"] = r.linf;
  d["l2"] = r.l2;
  d["cells"] = r.cells;
  return d;
}

py::dict cg_solve_dict(const CgSolve& r) {
  py::dict d;
  d["converged"] = r.converged;
  d["iterations"] = r.iterations;
  d["residual"] = r.residual;
  d["reason"] = r.reason;
  d["norm"] = r.norm;
  d["restarts"] = r.restarts;
  py::list hist;
  for (const auto& c : r.history) hist.append(py::make_tuple(c.iteration, c.linf, c.l2));
  d["history"] = hist;
  return d;
}

// What the single-GPU Poisson solvers (MultigridSolver, CgSolver, PcgSolver) offer alike.
template <typename Handle>
void def_poisson_methods(py::class_<Handle>& c) {
  c.def("geom", [](Handle& h) { return h.visit([](auto& s) { return s.geom(); }); })
      .def(
          "set_boundary",
          [](Handle& h, std::uintptr_t top, std::uintptr_t bottom, std::uintptr_t left, std::uintptr_t right) {
            h.visit([&](auto& s) {
              using T = typename std::decay_t<decltype(s)>::value_type;
              s.set_boundary(ptr<T>(top), ptr<T>(bottom), ptr<T>(left), ptr<T>(right));
            });
          },
          py::arg("top") = 0, py::arg("bottom") = 0, py::arg("left") = 0, py::arg("right") = 0,
          "device pointers to width (top, bottom) / height (left, right) boundary values; 0 leaves a side as it is")
      .def(
          "set_source",
          [](Handle& h, std::uintptr_t tile) {
            h.visit([&](auto& s) {
              using T = typename std::decay_t<decltype(s)>::value_type;
              s.set_source(ptr<T>(tile));
            });
          },
          py::arg("tile") = 0, "a device tile of geom() whose core holds g, or 0 (g = 0)")
      .def("set_field",
           [](Handle& h, std::uintptr_t tile) {
             h.visit([&](auto& s) {
               using T = typename std::decay_t<decltype(s)>::value_type;
               s.set_field(ptr<T>(tile));
             });
           })
      .def("field",
           [](Handle& h, std::uintptr_t tile) {
             h.visit([&](auto& s) {
               using T = typename std::decay_t<decltype(s)>::value_type;
               s.field(ptr<T>(tile));
             });
           })
      .def("residual",
           [](Handle& h) {
             const auto r = [&h] {
               py::gil_scoped_release nogil;
               return h.visit([](auto& s) { return s.residual(); });
             }();
             return residual_dict(r);
           })
      .def("graph_status", [](Handle& h) { return h.visit([](auto& s) { return s.graph_status(); }); })
      .def("note", [](Handle& h) { return h.visit([](auto& s) { return s.note(); }); });
}

// CgSolver and PcgSolver: the solve and the scalar block.
template <typename Handle>
void def_cg_methods(py::class_<Handle>& c, int max_iters, int check_every, const char* solve_doc) {
  c.def(
       "solve",
       [](Handle& h, double tol, int max_iters, const std::string& norm, int check_every) {
         CgSolve r;
         {
           py::gil_scoped_release nogil;
           r = h.visit([&](auto& s) { return s.solve(tol, max_iters, norm, check_every); });
         }
         return cg_solve_dict(r);
       },
       py::arg("tol"), py::arg("max_iters") = max_iters, py::arg("norm") = "l2", py::arg("check_every") = check_every,
       solve_doc)
      .def(
          "step",
          [](Handle& h, double lam, double theta, double tol, int max_iters, const std::string& norm, int check_every) {
            const kernels::HeatCoeffs hc = kernels::heat_coefficients(lam, theta);
            CgSolve r;
            {
              py::gil_scoped_release nogil;
              r = h.visit([&](auto& s) { return s.step(hc, tol, max_iters, norm, check_every); });
            }
            return cg_solve_dict(r);
          },
          py::arg("lam"), py::arg("theta"), py::arg("tol"), py::arg("max_iters") = max_iters, py::arg("norm") = "l2",
          py::arg("check_every") = check_every,
          "one implicit heat step (heat_coefficients(lam, theta)): solve() whose first start launch is the fused heat "
          "start, which makes the step's right-hand side from the field and the step source and stores it as g; "
          "raises unless the solver's weights are (0, c1)")
      .def(
          "set_step_source",
          [](Handle& h, std::uintptr_t tile) {
            h.visit([&](auto& s) {
              using T = typename std::decay_t<decltype(s)>::value_type;
              s.set_step_source(ptr<T>(tile));
            });
          },
          py::arg("tile") = 0, "a device tile of geom() whose core holds q = dt f of the steps to come, or 0 (none)")
      .def("scalars", [](Handle& h) { return h.visit([](auto& s) { return scalars_dict(s.scalars()); }); },
           "the device scalar block as a dict (a synchronising read)");
}

struct ExchangerHandle {
  DType dt;
  std::unique_ptr<HaloExchanger<float>> f;
  std::unique_ptr<HaloExchanger<double>> d;
};

}  // namespace

PYBIND11_MODULE(_mxs_hip, m) {
  m.doc() = "mxs HIP kernels (gfx950) and native runtime";

  m.def("device_count", []() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
      (void)hipGetLastError();
      return 0;
    }
    return n;
  });
  m.def("set_device", [](int d) { MXS_HIP_CHECK(hipSetDevice(d)); });
  m.def("device_sync", []() { MXS_HIP_CHECK(hipDeviceSynchronize()); });
  m.def("stream_sync", [](std::uintptr_t s) { MXS_HIP_CHECK(hipStreamSynchronize(strm(s))); });
  m.def("device_arch", [](int d) {
    hipDeviceProp_t p;
    MXS_HIP_CHECK(hipGetDeviceProperties(&p, d));
    return std::string(p.gcnArchName);
  });

  // ------------------------------------------------------------------ kernels
  m.def(
      "fill",
      [](std::uintptr_t p, index_t n, double v, const std::string& dt, std::uintptr_t s) {
        if (parse_dtype(dt) == DType::F32) kernels::fill<float>(ptr<float>(p), n, float(v), strm(s));
        else kernels::fill<double>(ptr<double>(p), n, v, strm(s));
      },
      py::arg("ptr"), py::arg("n"), py::arg("value"), py::arg("dtype"), py::arg("stream") = 0);
  m.def(
      "fill_region",
      [](std::uintptr_t p, const Array2D& r, double v, const std::string& dt, std::uintptr_t s) {
        if (parse_dtype(dt) == DType::F32) kernels::fill_region<float>(ptr<float>(p), r, float(v), strm(s));
        else kernels::fill_region<double>(ptr<double>(p), r, v, strm(s));
      },
      py::arg("ptr"), py::arg("region"), py::arg("value"), py::arg("dtype"), py::arg("stream") = 0);
  m.def(
      "fill_random",
      [](std::uintptr_t p, const TileGeom& g, index_t gx0, index_t gy0, index_t gw, std::uint64_t seed, double lo,
         double hi, const std::string& dt, std::uintptr_t s) {
        if (parse_dtype(dt) == DType::F32)
          kernels::fill_random<float>(ptr<float>(p), g, gx0, gy0, gw, seed, float(lo), float(hi), strm(s));
        else
          kernels::fill_random<double>(ptr<double>(p), g, gx0, gy0, gw, seed, lo, hi, strm(s));
      },
      py::arg("ptr"), py::arg("geom"), py::arg("global_x0"), py::arg("global_y0"), py::arg("global_width"),
      py::arg("seed"), py::arg("lo") = 0.0, py::arg("hi") = 1.0, py::arg("dtype") = "f32", py::arg("stream") = 0);
  m.def(
      "stencil5_rows",
      [](std::uintptr_t in, std::uintptr_t out, const TileGeom& g, index_t r0, index_t r1, double c0, double c1,
         const std::string& dt, std::uintptr_t s, const std::string& variant) {
        kernels::Stencil5Coeffs c{c0, c1};
        const auto v = parse_variant(variant);
        if (parse_dtype(dt) == DType::F32)
          kernels::stencil5_rows<float>(ptr<float>(in), ptr<float>(out), g, r0, r1, c, strm(s), v);
        else
          kernels::stencil5_rows<double>(ptr<double>(in), ptr<double>(out), g, r0, r1, c, strm(s), v);
      },
      py::arg("src"), py::arg("dst"), py::arg("geom"), py::arg("row_begin"), py::arg("row_end"),
      py::arg("c_center") = 0.2, py::arg("c_neighbor") = 0.2, py::arg("dtype") = "f32", py::arg("stream") = 0,
      py::arg("variant") = "auto");
  m.def(
      "auto_time_block",
      [](index_t w, index_t h, const std::string& dt, bool sum_form) {
        return kernels::auto_time_block(w, h, parse_dtype(dt) == DType::F32 ? 4 : 8, sum_form);
      },
      py::arg("width"), py::arg("height"), py::arg("dtype") = "f32", py::arg("sum_form") = true,
      "measured default Jacobi steps per pass / halo exchange for a tile");
  m.attr("MAX_TIME_BLOCK") = kernels::kMaxTimeBlock;
  m.attr("DEFAULT_CHECK_BLOCKS") = kDefaultCheckBlocks;
  m.attr("MAX_TIME_BLOCK_DEEP") = kernels::kMaxTimeBlockDeep;
  m.def(
      "last_stencil_dispatch", [] { return std::string(kernels::last_stencil_dispatch()); },
      "kernel form chosen by the most recent stencil launcher (e.g. 'stream_balanced_rot')");
  m.def("device_cu_count", &device_cu_count, "compute units of the current HIP device");
  m.def("set_gpu_share", &kernels::set_gpu_share, py::arg("processes"),
        "processes sharing this GPU: persistent stencil kernels take 1/processes of the chip");
  m.def("gpu_share", &kernels::gpu_share);
  m.def("set_pipe_joint", &kernels::set_pipe_joint, py::arg("on"),
        "joint stage-1 windows in the fp32 two-stage pipeline (default on; bitwise equal output)");
  m.def("pipe_joint", &kernels::pipe_joint);
  m.def("set_pipe_lag1", &kernels::set_pipe_lag1, py::arg("on"),
        "ascending level order in the joint fp32 pipeline where it pays (default on; bitwise equal output)");
  m.def("pipe_lag1", &kernels::pipe_lag1);
  m.def("set_pipe_split", &kernels::set_pipe_split, py::arg("on"),
        "split a narrow last column group of the fp32 S = 24 pass into two half-height sub-groups (default on; "
        "bitwise equal output)");
  m.def("pipe_split", &kernels::pipe_split);
  m.def("last_pipe_split", &kernels::last_pipe_split,
        "whether the most recent stencil launch was a pipeline pass that split its last group");
  m.def("set_pipe_block_prio", &kernels::set_pipe_block_prio, py::arg("on"),
        "in-block progress priority of the fp32 S = 20 / 24 joint pipeline passes (default on; bitwise equal output)");
  m.def("pipe_block_prio", &kernels::pipe_block_prio);
  m.def("last_pipe_block_prio", &kernels::last_pipe_block_prio,
        "whether the most recent stencil launch was a pipeline pass with the in-block progress priority");
  m.def("set_pipe_balanced", &kernels::set_pipe_balanced, py::arg("on"),
        "fill-aware workgroup shares in the pipeline passes (default on; bitwise equal output)");
  m.def("pipe_balanced", &kernels::pipe_balanced_on);
  m.def(
      "absmax",
      [](std::uintptr_t x, index_t n, const std::string& dt) {
        double r = 0;
        if (parse_dtype(dt) == DType::F32) {
          DeviceBuffer<float> o(1);
          kernels::absmax<float>(ptr<float>(x), n, o.get(), nullptr);
          float h = 0;
          MXS_HIP_CHECK(hipMemcpy(&h, o.get(), sizeof(float), hipMemcpyDeviceToHost));
          r = h;
        } else {
          DeviceBuffer<double> o(1);
          kernels::absmax<double>(ptr<double>(x), n, o.get(), nullptr);
          MXS_HIP_CHECK(hipMemcpy(&r, o.get(), sizeof(double), hipMemcpyDeviceToHost));
        }
        return r;
      },
      py::arg("x"), py::arg("n"), py::arg("dtype") = "f32", "max |x[i]| (device reduction; NaN if any is NaN)");
  m.def(
      "stencil5_residual",
      [](std::uintptr_t x, const TileGeom& g, double c0, double c1, const std::string& dt, std::uintptr_t s,
         std::uintptr_t source) {
        kernels::Stencil5Coeffs c{c0, c1};
        const index_t grid = kernels::residual_grid_size(g);
        DeviceBuffer<double> buf(2 + 2 * grid);
        DeviceBuffer<unsigned> counter(1);
        auto* norms = reinterpret_cast<kernels::ResidualNorms*>(buf.get());
        if (parse_dtype(dt) == DType::F32)
          kernels::stencil5_residual<float>(ptr<float>(x), g, c, norms, buf.get() + 2, counter.get(), strm(s),
                                            ptr<float>(source));
        else
          kernels::stencil5_residual<double>(ptr<double>(x), g, c, norms, buf.get() + 2, counter.get(), strm(s),
                                             ptr<double>(source));
        kernels::ResidualNorms h{0.0, 0.0};
        MXS_HIP_CHECK(hipMemcpyAsync(&h, norms, sizeof(h), hipMemcpyDeviceToHost, strm(s)));
        MXS_HIP_CHECK(hipStreamSynchronize(strm(s)));
        return py::make_tuple(h.linf, h.sumsq);
      },
      py::arg("src"), py::arg("geom"), py::arg("c_center") = 0.2, py::arg("c_neighbor") = 0.2,
      py::arg("dtype") = "f32", py::arg("stream") = 0, py::arg("source") = 0,
      "(max |r|, sum r^2) of the Jacobi residual r = A u - u over the core of a ghost-ring tile "
      "(reads the core and the ring cells beside it only; synchronises the stream); source: a tile of the same "
      "geometry whose core holds g, then r = A u + g - u (0: none)");
  m.def(
      "residual_kernel_times",
      [](std::uintptr_t x, const TileGeom& g, double c0, double c1, const std::string& dt, int reps) {
        // Measurements: `reps` event-timed pairs (stencil5_residual on the tile,
        // absmax over the same buffer), scratch allocated once, one stream.
        kernels::Stencil5Coeffs c{c0, c1};
        const bool f32 = parse_dtype(dt) == DType::F32;
        const index_t grid = kernels::residual_grid_size(g);
        DeviceBuffer<double> buf(2 + 2 * grid), amax(1);
        DeviceBuffer<unsigned> counter(1);
        auto* norms = reinterpret_cast<kernels::ResidualNorms*>(buf.get());
        Stream st(true, 0);
        Event e0(true), e1(true), e2(true);
        py::list res, abs;
        for (int i = 0; i < reps; ++i) {
          e0.record(st.get());
          if (f32) kernels::stencil5_residual<float>(ptr<float>(x), g, c, norms, buf.get() + 2, counter.get(), st.get());
          else kernels::stencil5_residual<double>(ptr<double>(x), g, c, norms, buf.get() + 2, counter.get(), st.get());
          e1.record(st.get());
          if (f32) kernels::absmax<float>(ptr<float>(x), g.alloc_elems(), reinterpret_cast<float*>(amax.get()), st.get());
          else kernels::absmax<double>(ptr<double>(x), g.alloc_elems(), amax.get(), st.get());
          e2.record(st.get());
          MXS_HIP_CHECK(hipStreamSynchronize(st.get()));
          res.append(double(e1.since(e0)));
          abs.append(double(e2.since(e1)));
        }
        py::dict d;
        d["residual_ms"] = res;
        d["absmax_ms"] = abs;
        d["workgroups"] = grid;
        return d;
      },
      py::arg("src"), py::arg("geom"), py::arg("c_center") = 0.2, py::arg("c_neighbor") = 0.2,
      py::arg("dtype") = "f32", py::arg("reps") = 20,
      "measurements: event-timed (residual, absmax) kernel pairs over one tile, ms per launch");
  m.def(
      "stencil5_chunk_pass",
      [](std::uintptr_t in, std::uintptr_t out, const TileGeom& g, int steps, double c0, double c1,
         const std::string& dt, int outer_wgs, std::uintptr_t s, bool sum_form, double range, double lead_frac,
         const std::string& part) -> py::object {
        // One interior-first pass (tests / tuning): the inner and the outer
        // chunk lists of kernels::make_halo_last_schedule as two launches of the
        // chunk-list kernel on one stream. The tables live for the call, so the
        // launches are synchronised before return. part: "both", or "inner" /
        // "outer" alone (timing one set against the one-launch pass).
        MXS_CHECK(part == "both" || part == "inner" || part == "outer", "stencil5_chunk_pass: part both|inner|outer");
        kernels::Stencil5Coeffs c{c0, c1, sum_form, range};
        auto run = [&](auto tag) -> py::object {
          using T = decltype(tag);
          kernels::ChunkPassShape sh;
          if (!kernels::chunk_pass_shape<T>(g, steps, c, &sh) || sh.blocks < 2) return py::none();
          std::vector<std::uint8_t> ghost(size_t(sh.groups), 0);
          for (index_t k = 0; k < sh.groups; ++k) {
            const index_t x0 = k * sh.owg - sh.read_lead;
            ghost[size_t(k)] = (x0 < 0 || x0 + sh.read_span > g.width) ? 1 : 0;
          }
          const auto hl = kernels::make_halo_last_schedule(sh.groups, g.height, sh.blocks, sh.fill, steps, ghost,
                                                           outer_wgs, lead_frac, 0, sh.blocks % kNumXCDs == 0 ? kNumXCDs : 1,
                                                           32);
          DeviceBuffer<kernels::PassChunk> ti(index_t(hl.inner.table.size())), to(index_t(hl.outer.table.size()));
          MXS_HIP_CHECK(hipMemcpy(ti.get(), hl.inner.table.data(), ti.bytes(), hipMemcpyHostToDevice));
          MXS_HIP_CHECK(hipMemcpy(to.get(), hl.outer.table.data(), to.bytes(), hipMemcpyHostToDevice));
          kernels::ChunkPassShape si = sh, so = sh;
          si.blocks = hl.inner.blocks;
          so.blocks = hl.outer.blocks;
          Event e0(true), e1(true);
          e0.record(strm(s));
          if (part != "outer")
            kernels::stencil5_chunk_pass<T>(ptr<T>(in), ptr<T>(out), g, c, si, ti.get(), hl.inner.entries, strm(s));
          if (part != "inner")
            kernels::stencil5_chunk_pass<T>(ptr<T>(in), ptr<T>(out), g, c, so, to.get(), hl.outer.entries, strm(s));
          e1.record(strm(s));
          MXS_HIP_CHECK(hipStreamSynchronize(strm(s)));
          py::dict d;
          d["inner_blocks"] = hl.inner.blocks;
          d["outer_blocks"] = hl.outer.blocks;
          d["check"] = kernels::check_halo_last_schedule(hl, sh.groups, g.height, steps, ghost);
          d["js0"] = sh.form.s0;
          d["lag1"] = sh.form.lag1;
          d["fill"] = sh.fill;
          d["band"] = hl.band;
          d["inner_cost"] = hl.inner_cost;
          d["outer_cost"] = hl.outer_cost;
          d["serial_cost"] = hl.serial_cost;
          d["kernel_us"] = double(e1.since(e0)) * 1000.0;
          return d;
        };
        return parse_dtype(dt) == DType::F32 ? run(float{}) : run(double{});
      },
      py::arg("src"), py::arg("dst"), py::arg("geom"), py::arg("steps"), py::arg("c_center") = 0.2,
      py::arg("c_neighbor") = 0.2, py::arg("dtype") = "f32", py::arg("outer_wgs") = 0, py::arg("stream") = 0,
      py::arg("sum_form") = true, py::arg("range") = -1.0, py::arg("lead_frac") = 0.12, py::arg("part") = "both",
      "one interior-first pass (inner + outer chunk lists) over the core of a ghost-ring tile (None: no "
      "chunk-list form for this depth); sum_form / range as for stencil5_tb; lead_frac: the exchange's share "
      "of the pass the schedule assumes; part: both, inner or outer alone");
  m.def("last_pipe_lag1", &kernels::last_pipe_lag1,
        "whether the most recent stencil launch was a pipeline pass in ascending level order");
  m.def(
      "last_pipe_form",
      [] {
        const kernels::PipeForm f = kernels::last_pipe_form();
        py::dict d;
        d["js0"] = f.joint ? f.s0 : 0;
        d["lag1"] = f.lag1;
        d["split"] = kernels::last_pipe_split();
        d["block_prio"] = kernels::last_pipe_block_prio();
        return d;
      },
      "the most recent stencil launch as a pipeline pass (one launch or chunk list): js0 (stage-0 levels of the "
      "joint windows, 0: per-strip layout or no pipeline pass), lag1 (level-order mask), split (narrow last group), "
      "block_prio (in-block progress priority)");
  m.def(
      "stencil5_tb_held",
      [](std::uintptr_t in, std::uintptr_t out, const TileGeom& g, int steps, index_t x0, index_t x1, index_t y0,
         index_t y1, double c0, double c1, unsigned hold, const std::string& dt, std::uintptr_t s) {
        kernels::Stencil5Coeffs c{c0, c1, false, -1.0};
        if (parse_dtype(dt) == DType::F32)
          kernels::stencil5_tb_held<float>(ptr<float>(in), ptr<float>(out), g, steps, x0, x1, y0, y1, c, hold, strm(s));
        else
          kernels::stencil5_tb_held<double>(ptr<double>(in), ptr<double>(out), g, steps, x0, x1, y0, y1, c, hold,
                                            strm(s));
      },
      py::arg("src"), py::arg("dst"), py::arg("geom"), py::arg("steps"), py::arg("x0"), py::arg("x1"), py::arg("y0"),
      py::arg("y1"), py::arg("c_center") = 0.2, py::arg("c_neighbor") = 0.2, py::arg("hold") = 15u,
      py::arg("dtype") = "f32", py::arg("stream") = 0,
      "S Jacobi steps over [x0, x1) x [y0, y1) of a ghost-ring tile beside fixed edges: cells outside the core on a "
      "held side (hold: HOLD_TOP | HOLD_BOTTOM | HOLD_LEFT | HOLD_RIGHT) keep their input value at every level; "
      "per-step form, bitwise equal to S single steps");
  auto level_table = [](const std::vector<double>& center, const std::vector<double>& neighbor) {
    if (center.size() != neighbor.size() || center.empty() || int(center.size()) > kernels::kMaxLevels)
      throw std::invalid_argument("a level table takes 1.." + std::to_string(kernels::kMaxLevels) +
                                  " (center, neighbor) pairs");
    kernels::LevelTable t;
    t.n = int(center.size());
    for (int l = 0; l < t.n; ++l) {
      t.center[l] = center[size_t(l)];
      t.neighbor[l] = neighbor[size_t(l)];
    }
    return t;
  };
  m.def(
      "stencil5_tb_levels",
      [level_table](std::uintptr_t in, std::uintptr_t out, const TileGeom& g, index_t x0, index_t x1, index_t y0,
                    index_t y1, const std::vector<double>& center, const std::vector<double>& neighbor,
                    const std::string& dt, std::uintptr_t s, std::uintptr_t corr) {
        const kernels::LevelTable t = level_table(center, neighbor);
        if (parse_dtype(dt) == DType::F32)
          kernels::stencil5_tb_levels<float>(ptr<float>(in), ptr<float>(out), g, x0, x1, y0, y1, t, ptr<float>(corr),
                                             strm(s));
        else
          kernels::stencil5_tb_levels<double>(ptr<double>(in), ptr<double>(out), g, x0, x1, y0, y1, t,
                                              ptr<double>(corr), strm(s));
      },
      py::arg("src"), py::arg("dst"), py::arg("geom"), py::arg("x0"), py::arg("x1"), py::arg("y0"), py::arg("y1"),
      py::arg("center"), py::arg("neighbor"), py::arg("dtype") = "f32", py::arg("stream") = 0, py::arg("corr") = 0,
      "one pass of len(center) levels over [x0, x1) x [y0, y1) of a ghost-ring tile, level l with (center[l], "
      "neighbor[l]): the per-step stencil5_tb (no wrap) with a level table; fp32 20 / 24 levels, fp64 12 / 16");
  m.def(
      "stencil5_tb_held_levels",
      [level_table](std::uintptr_t in, std::uintptr_t out, const TileGeom& g, index_t x0, index_t x1, index_t y0,
                    index_t y1, const std::vector<double>& center, const std::vector<double>& neighbor, unsigned hold,
                    const std::string& dt, std::uintptr_t s, std::uintptr_t corr) {
        const kernels::LevelTable t = level_table(center, neighbor);
        if (parse_dtype(dt) == DType::F32)
          kernels::stencil5_tb_held_levels<float>(ptr<float>(in), ptr<float>(out), g, x0, x1, y0, y1, t, hold,
                                                  ptr<float>(corr), strm(s));
        else
          kernels::stencil5_tb_held_levels<double>(ptr<double>(in), ptr<double>(out), g, x0, x1, y0, y1, t, hold,
                                                   ptr<double>(corr), strm(s));
      },
      py::arg("src"), py::arg("dst"), py::arg("geom"), py::arg("x0"), py::arg("x1"), py::arg("y0"), py::arg("y1"),
      py::arg("center"), py::arg("neighbor"), py::arg("hold") = 15u, py::arg("dtype") = "f32", py::arg("stream") = 0,
      py::arg("corr") = 0,
      "stencil5_tb_held with a level table: level l runs (center[l], neighbor[l]); cells outside the core on a held "
      "side keep their input value at every level");
  m.def(
      "source_axpy",
      [](std::uintptr_t tile, std::uintptr_t src, const TileGeom& g, double w, const std::string& dt, std::uintptr_t s) {
        if (parse_dtype(dt) == DType::F32) kernels::source_axpy<float>(ptr<float>(tile), ptr<float>(src), g, w, strm(s));
        else kernels::source_axpy<double>(ptr<double>(tile), ptr<double>(src), g, w, strm(s));
      },
      py::arg("tile"), py::arg("src"), py::arg("geom"), py::arg("w"), py::arg("dtype") = "f32", py::arg("stream") = 0,
      "tile core += T(w) * src core: the product rounded, then the sum (the build step of a source's correction)");
  m.attr("HOLD_TOP") = unsigned(kernels::kHoldTop);
  m.attr("HOLD_BOTTOM") = unsigned(kernels::kHoldBottom);
  m.attr("HOLD_LEFT") = unsigned(kernels::kHoldLeft);
  m.attr("HOLD_RIGHT") = unsigned(kernels::kHoldRight);
  m.def(
      "stencil5_tb",
      [](std::uintptr_t in, std::uintptr_t out, const TileGeom& g, int steps, index_t x0, index_t x1, index_t y0,
         index_t y1, double c0, double c1, bool wrap, const std::string& dt, std::uintptr_t s,
         const std::string& variant, bool sum_form, double range) {
        kernels::Stencil5Coeffs c{c0, c1, sum_form, range};
        const kernels::StencilVariant v = parse_variant(variant);
        if (parse_dtype(dt) == DType::F32)
          kernels::stencil5_tb<float>(ptr<float>(in), ptr<float>(out), g, steps, x0, x1, y0, y1, c, wrap, strm(s), v);
        else
          kernels::stencil5_tb<double>(ptr<double>(in), ptr<double>(out), g, steps, x0, x1, y0, y1, c, wrap, strm(s),
                                       v);
      },
      py::arg("src"), py::arg("dst"), py::arg("geom"), py::arg("steps"), py::arg("x0"), py::arg("x1"), py::arg("y0"),
      py::arg("y1"), py::arg("c_center") = 0.2, py::arg("c_neighbor") = 0.2, py::arg("wrap") = false,
      py::arg("dtype") = "f32", py::arg("stream") = 0, py::arg("variant") = "auto", py::arg("sum_form") = true,
      py::arg("range") = -1.0,
      "S Jacobi steps over [x0, x1) x [y0, y1). sum_form: allow the fast forms — the sum form (c_center == "
      "c_neighbor) or the scaled form (unequal, c_neighbor != 0) — within their bounds (kernels::fast_form_safe: "
      "|c_center| + 4 |c_neighbor| <= 1, c_neighbor^S normal, range (4 + |c_center / c_neighbor|)^S < max / 4). "
      "range: a bound on max|u| of the input (< 0: unknown; then only forms growing no faster than the sum form "
      "run fast, under its contract max|u| 5^S < max / 4); otherwise the per-step form");
  m.def(
      "streams_concurrent",
      [](std::uintptr_t a, std::uintptr_t b) { return kernels::streams_concurrent(strm(a), strm(b)); },
      py::arg("a"), py::arg("b"), py::call_guard<py::gil_scoped_release>(),
      "whether work on stream b runs while a kernel on stream a still runs (different hardware queues)");
  m.def(
      "clock_stamp",
      [](std::uintptr_t out, std::uintptr_t s) { kernels::clock_stamp(ptr<unsigned long long>(out), strm(s)); },
      py::arg("out"), py::arg("stream") = 0,
      "kClockStampWgs workgroups write (XCC id, shader clock cycles, wall clock ticks) to out[3b..3b+2] "
      "(int64 device buffer of 3 * clock_stamp_slots())");
  m.def("clock_stamp_slots", [] { return kernels::kClockStampWgs; });
  m.def(
      "wall_clock_rate_khz",
      [] {
        int dev = 0, khz = 0;
        MXS_HIP_CHECK(hipGetDevice(&dev));
        MXS_HIP_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev));
        return khz;
      },
      "rate of wall_clock64() on the current device (kHz)");
  m.def(
      "spin_delay", [](double us, std::uintptr_t s) { kernels::spin_delay(us, strm(s)); }, py::arg("us"),
      py::arg("stream") = 0, "a single-wave kernel holding `stream` for `us` microseconds (wire-time rehearsal)");
  m.def(
      "stencil5_rect",
      [](std::uintptr_t in, std::uintptr_t out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
         double c0, double c1, const std::string& dt, std::uintptr_t s) {
        kernels::Stencil5Coeffs c{c0, c1};
        if (parse_dtype(dt) == DType::F32)
          kernels::stencil5_rect<float>(ptr<float>(in), ptr<float>(out), g, x0, x1, y0, y1, c, strm(s));
        else
          kernels::stencil5_rect<double>(ptr<double>(in), ptr<double>(out), g, x0, x1, y0, y1, c, strm(s));
      },
      py::arg("src"), py::arg("dst"), py::arg("geom"), py::arg("x0"), py::arg("x1"), py::arg("y0"), py::arg("y1"),
      py::arg("c_center") = 0.2, py::arg("c_neighbor") = 0.2, py::arg("dtype") = "f32", py::arg("stream") = 0);
  m.def(
      "stencil_box",
      [](std::uintptr_t in, std::uintptr_t out, const TileGeom& g, index_t x0, index_t x1, index_t y0, index_t y1,
         int radius, const std::vector<float>& w, const std::string& dt, std::uintptr_t s) {
        const auto b = make_box(radius, w);
        if (parse_dtype(dt) == DType::F32)
          kernels::stencil_box<float>(ptr<float>(in), ptr<float>(out), g, x0, x1, y0, y1, b, strm(s));
        else
          kernels::stencil_box<double>(ptr<double>(in), ptr<double>(out), g, x0, x1, y0, y1, b, strm(s));
      },
      py::arg("src"), py::arg("dst"), py::arg("geom"), py::arg("x0"), py::arg("x1"), py::arg("y0"), py::arg("y1"),
      py::arg("radius"), py::arg("weights"), py::arg("dtype") = "f32", py::arg("stream") = 0);
  m.def("dot_grid_size", [](index_t n) { return kernels::dot_grid_size(n, kernels::kDotBlock); });
  m.def(
      "dot",
      [](std::uintptr_t x, std::uintptr_t y, index_t n, std::uintptr_t out, std::uintptr_t partials,
         std::uintptr_t counter, const std::string& reduce, const std::string& dt, const std::string& acc, int grid,
         std::uintptr_t s) {
        const auto mode = parse_reduce(reduce);
        const DType d = parse_dtype(dt), a = parse_dtype(acc);
        if (d == DType::F32 && a == DType::F32)
          kernels::dot<float, float>(ptr<float>(x), ptr<float>(y), n, ptr<float>(out), ptr<float>(partials),
                                     ptr<unsigned>(counter), mode, grid, strm(s));
        else if (d == DType::F32)
          kernels::dot<float, double>(ptr<float>(x), ptr<float>(y), n, ptr<double>(out), ptr<double>(partials),
                                      ptr<unsigned>(counter), mode, grid, strm(s));
        else if (a == DType::F64)
          kernels::dot<double, double>(ptr<double>(x), ptr<double>(y), n, ptr<double>(out), ptr<double>(partials),
                                       ptr<unsigned>(counter), mode, grid, strm(s));
        else
          throw std::invalid_argument("f64 inputs need an f64 accumulator");
      },
      py::arg("x"), py::arg("y"), py::arg("n"), py::arg("out"), py::arg("partials"), py::arg("counter"),
      py::arg("reduce") = "single-pass", py::arg("dtype") = "f64", py::arg("acc") = "f64", py::arg("grid") = 0,
      py::arg("stream") = 0);

  // ------------------------------------------------------------------ RCCL
  m.def(
      "set_comm_timeout", [](double s) { comm_timeout() = s; }, py::arg("seconds"),
      "communication watchdog: waits on RCCL streams / IPC peers fail after this many seconds (0 = forever)");
  m.def("comm_timeout", [] { return comm_timeout(); });
  m.def("experiments_build", [] { return kExperimentsBuild; },
        "whether this build honours the MXS_* tuning environment knobs (-DMXS_EXPERIMENTS=ON)");
  py::class_<RcclComm>(m, "RcclComm")
      .def(py::init([](py::bytes uid, int nranks, int rank) {
             return std::make_unique<RcclComm>(std::string(uid), nranks, rank);
           }),
           py::arg("unique_id"), py::arg("nranks"), py::arg("rank"), py::call_guard<py::gil_scoped_release>())
      .def_static("make_unique_id", []() { return py::bytes(RcclComm::make_unique_id()); })
      .def_property_readonly("rank", &RcclComm::rank)
      .def_property_readonly("size", &RcclComm::size)
      .def("count", &RcclComm::count, "ranks the communicator spans (ncclCommCount)")
      .def("device", &RcclComm::device, "HIP device of this rank's end (ncclCommCuDevice)")
      .def("healthy",
           [](const RcclComm& c) {
             std::string msg;
             const bool ok = c.healthy(&msg);
             return py::make_tuple(ok, msg);
           })
      .def("abort", &RcclComm::abort, py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("aborted", &RcclComm::aborted)
      .def(
          "wait",
          [](const RcclComm& c, std::uintptr_t s, const std::string& what) { c.wait(strm(s), what.c_str()); },
          py::arg("stream") = 0, py::arg("what") = "RCCL stream", py::call_guard<py::gil_scoped_release>(),
          "wait for `stream` under the communication watchdog (set_comm_timeout)")
      .def(
          "allreduce_sum",
          [](const RcclComm& c, std::uintptr_t send, std::uintptr_t recv, size_t count, const std::string& dt,
             std::uintptr_t s) {
            if (parse_dtype(dt) == DType::F32) c.allreduce_sum<float>(ptr<float>(send), ptr<float>(recv), count, strm(s));
            else c.allreduce_sum<double>(ptr<double>(send), ptr<double>(recv), count, strm(s));
          },
          py::arg("send"), py::arg("recv"), py::arg("count"), py::arg("dtype"), py::arg("stream") = 0)
      .def(
          "send_bytes",
          [](const RcclComm& c, std::uintptr_t buf, size_t n, int peer, std::uintptr_t s) {
            c.send<unsigned char>(ptr<unsigned char>(buf), n, peer, strm(s));
          },
          py::arg("buf"), py::arg("nbytes"), py::arg("peer"), py::arg("stream") = 0)
      .def(
          "recv_bytes",
          [](const RcclComm& c, std::uintptr_t buf, size_t n, int peer, std::uintptr_t s) {
            c.recv<unsigned char>(ptr<unsigned char>(buf), n, peer, strm(s));
          },
          py::arg("buf"), py::arg("nbytes"), py::arg("peer"), py::arg("stream") = 0)
      .def("group_start", &RcclComm::group_start)
      .def("group_end", &RcclComm::group_end);

  // ------------------------------------------------------------------ halo
  py::enum_<HaloBackend>(m, "HaloBackend")
      .value("LOCAL", HaloBackend::Local)
      .value("RCCL", HaloBackend::Rccl)
      .value("IPC", HaloBackend::Ipc);
  py::class_<ExchangerHandle>(m, "HaloExchanger")
      .def(py::init([](const HaloPlan& plan, HaloBackend b, const RcclComm* comm, const std::string& dt,
                       py::object bootstrap, int world_size) {
             auto h = std::make_unique<ExchangerHandle>();
             h->dt = parse_dtype(dt);
             HaloBootstrap boot;
             boot.rank = plan.rank;
             boot.world_size = world_size;
             boot.allgather = wrap_allgather(bootstrap);
             if (h->dt == DType::F32) h->f = std::make_unique<HaloExchanger<float>>(plan, b, comm, &boot);
             else h->d = std::make_unique<HaloExchanger<double>>(plan, b, comm, &boot);
             return h;
           }),
           py::arg("plan"), py::arg("backend"), py::arg("comm") = nullptr, py::arg("dtype") = "f32",
           py::arg("bootstrap") = py::none(), py::arg("world_size") = 1, py::keep_alive<1, 4>())
      .def("check", [](const ExchangerHandle& h) { h.dt == DType::F32 ? h.f->check() : h.d->check(); })
      .def(
          "exchange",
          [](ExchangerHandle& h, std::uintptr_t tile, std::uintptr_t s) {
            if (h.dt == DType::F32) h.f->exchange(ptr<float>(tile), strm(s));
            else h.d->exchange(ptr<double>(tile), strm(s));
          },
          py::arg("tile"), py::arg("stream") = 0)
      .def("wire_bytes", [](const ExchangerHandle& h) { return h.dt == DType::F32 ? h.f->wire_bytes() : h.d->wire_bytes(); });

  // ------------------------------------------------------------------ solver
  py::enum_<StencilKind>(m, "StencilKind").value("JACOBI5", StencilKind::Jacobi5).value("BOX", StencilKind::Box);
  py::class_<SolverHandle>(m, "StencilSolver")
      .def(py::init([](const CartTopology& topo, int rank, const TileGeom& tile, std::uintptr_t a, std::uintptr_t b,
                       const RcclComm* comm, const std::string& dt, HaloBackend backend, bool overlap,
                       bool use_graph, bool loopback_self, StencilKind kind, double c0, double c1, int box_radius,
                       const std::vector<float>& box_w, const std::string& variant, bool fuse_periodic, int time_block,
                       py::object bootstrap, int graph_supersteps, bool sum_form, const std::string& direct_halo,
                       double graph_max_superstep_us, const std::string& opening, bool rehearse_peers,
                       double min_gain, int halo_max_ctas, int main_priority, int side_priority,
                       double wire_delay_us, const std::string& direct_engine, const std::string& steady,
                       bool block_fixed_edges, const std::string& relaxation, index_t global_width,
                       index_t global_height, bool source) {
             SolverConfig cfg;
             cfg.source = source;
             cfg.block_fixed_edges = block_fixed_edges;
             if (relaxation == "none") cfg.relaxation = Relaxation::None;
             else if (relaxation == "chebyshev") cfg.relaxation = Relaxation::Chebyshev;
             else throw std::invalid_argument("relaxation must be none or chebyshev, got '" + relaxation + "'");
             cfg.global_width = global_width;
             cfg.global_height = global_height;
             cfg.steady = parse_opening(steady, "steady");
             if (direct_engine == "kernel") cfg.direct_engine = PushEngine::Kernel;
             else if (direct_engine == "copy-engine") cfg.direct_engine = PushEngine::CopyEngine;
             else throw std::invalid_argument("direct_engine must be kernel or copy-engine, got '" + direct_engine + "'");
             cfg.main_priority = main_priority;
             cfg.side_priority = side_priority;
             cfg.halo_max_ctas = halo_max_ctas;
             cfg.wire_delay_us = wire_delay_us;
             cfg.opening = parse_opening(opening, "opening");
             cfg.rehearse_peers = rehearse_peers;
             cfg.min_gain = min_gain;
             cfg.graph_max_superstep_us = graph_max_superstep_us;
             cfg.bootstrap = wrap_allgather(bootstrap);
             cfg.graph_supersteps = graph_supersteps;
             if (direct_halo == "off") cfg.direct = DirectHalo::Off;
             else if (direct_halo == "on") cfg.direct = DirectHalo::On;
             else if (direct_halo == "validate") cfg.direct = DirectHalo::Validate;
             else throw std::invalid_argument("direct_halo must be off, on or validate, got '" + direct_halo + "'");
             cfg.backend = backend;
             cfg.overlap = overlap;
             cfg.use_graph = use_graph;
             cfg.loopback_self = loopback_self;
             cfg.fuse_periodic_self = fuse_periodic;
             cfg.time_block = time_block;
             cfg.kind = kind;
             cfg.coeffs = {c0, c1, sum_form};
             cfg.variant = parse_variant(variant);
             if (kind == StencilKind::Box) cfg.box = make_box(box_radius, box_w);
             auto h = std::make_unique<SolverHandle>();
             h->dt = parse_dtype(dt);
             if (h->dt == DType::F32)
               h->f = std::make_unique<StencilSolver<float>>(topo, rank, tile, ptr<float>(a), ptr<float>(b), comm, cfg);
             else
               h->d = std::make_unique<StencilSolver<double>>(topo, rank, tile, ptr<double>(a), ptr<double>(b), comm,
                                                              cfg);
             return h;
           }),
           py::arg("topo"), py::arg("rank"), py::arg("tile"), py::arg("buf_a"), py::arg("buf_b"),
           py::arg("comm") = nullptr, py::arg("dtype") = "f32", py::arg("backend") = HaloBackend::Local,
           py::arg("overlap") = true, py::arg("use_graph") = true, py::arg("loopback_self") = false,
           py::arg("kind") = StencilKind::Jacobi5, py::arg("c_center") = 0.2, py::arg("c_neighbor") = 0.2,
           py::arg("box_radius") = 1, py::arg("box_weights") = std::vector<float>{}, py::arg("variant") = "auto",
           py::arg("fuse_periodic") = true, py::arg("time_block") = 1, py::arg("bootstrap") = py::none(),
           py::arg("graph_supersteps") = 0, py::arg("sum_form") = true, py::arg("direct_halo") = "off",
           py::arg("graph_max_superstep_us") = 150.0, py::arg("opening") = "auto", py::arg("rehearse_peers") = false,
           py::arg("min_gain") = 0.0, py::arg("halo_max_ctas") = 0, py::arg("main_priority") = -1,
           py::arg("side_priority") = 0, py::arg("wire_delay_us") = 0.0, py::arg("direct_engine") = "kernel",
           py::arg("steady") = "auto", py::arg("block_fixed_edges") = false, py::arg("relaxation") = "none",
           py::arg("global_width") = 0, py::arg("global_height") = 0, py::arg("source") = false,
           py::keep_alive<1, 7>())
      .def(
          "set_source",
          [](SolverHandle& h, std::uintptr_t g_tile) {
            if (h.dt == DType::F32) h.f->set_source(ptr<float>(g_tile));
            else h.d->set_source(ptr<double>(g_tile));
          },
          py::arg("g_tile"), py::call_guard<py::gil_scoped_release>(),
          "collective: take the source term from a device tile of the solver's geometry whose core holds g "
          "(u' = A u + g); 0 clears it. Builds the cycle's correction, drops captured graphs, ends like field_changed()")
      .def(
          "source_correction",
          [](SolverHandle& h) {
            return h.visit([](auto& s) { return reinterpret_cast<std::uintptr_t>(s.source_correction()); });
          },
          "device address of the cycle's correction tile G (0 while no source is set)")
      .def(
          "copy_source_correction",
          [](SolverHandle& h, std::uintptr_t dst) {
            return h.visit([dst](auto& s) {
              if (!s.source_correction()) return false;
              s.synchronize();
              using E = std::remove_const_t<std::remove_pointer_t<decltype(s.source_correction())>>;
              MXS_HIP_CHECK(hipMemcpy(reinterpret_cast<void*>(dst), s.source_correction(),
                                      size_t(s.plan().tile.alloc_elems()) * sizeof(E), hipMemcpyDeviceToDevice));
              return true;
            });
          },
          py::arg("dst"), "copy the correction tile G into a device tile of the solver's geometry (false: no source set)")
      .def("source_set", [](SolverHandle& h) { return h.visit([](auto& s) { return s.source_set(); }); })
      .def("field_changed", [](SolverHandle& h) { h.visit([](auto& s) { s.field_changed(); }); },
           "the caller wrote the field: re-exchange the ghost ring and re-check the sum form's range next run")
      .def(
          "halo_last", [](SolverHandle& h, int S) { return h.visit([S](auto& s) { return s.halo_last(S); }); },
          py::arg("S"), "whether a call's opening super-step of depth S runs interior-first on this rank")
      .def(
          "force_opening",
          [](SolverHandle& h, const std::string& o) {
            const Opening op = parse_opening(o, "opening");
            h.visit([op](auto& s) { s.force_opening(op); });
          },
          py::arg("opening"),
          "paired measurements: the opening of the following calls (serial, interior-first, or auto = the one "
          "construction / prepare() chose); collective")
      .def(
          "force_steady",
          [](SolverHandle& h, const std::string& o) {
            const Opening op = parse_opening(o, "steady");
            h.visit([op](auto& s) { s.force_steady(op); });
          },
          py::arg("steady"), "paired measurements: the later super-steps' schedule of the following calls")
      .def("fixed_edge_note", [](SolverHandle& h) { return h.visit([](auto& s) { return s.fixed_edge_note(); }); },
           "fixed edges under time blocking: this rank's held sides and its interior / frame split ('' when inactive)")
      .def("held_sides", [](SolverHandle& h) { return h.visit([](auto& s) { return s.held_sides(); }); },
           "this rank's held sides (HOLD_TOP | HOLD_BOTTOM | HOLD_LEFT | HOLD_RIGHT bits; 0 when inactive)")
      .def("multi_rank", [](SolverHandle& h) { return h.visit([](auto& s) { return s.multi_rank(); }); },
           "whether the solver follows the peers' schedule (remote peers or a loopback rehearsal)")
      .def("schedule_times",
           [](SolverHandle& h) {
             return h.visit([](auto& s) {
               const OpeningRecord& o = s.opening_record();
               py::dict d;
               d["opening"] = to_string(o.choice);
               d["reason"] = o.reason;
               d["rule"] = o.rule;
               d["serial_ms"] = o.decision.baseline_ms;
               d["interior_first_ms"] = o.decision.candidate_ms;
               d["serial_iqr_ms"] = o.decision.baseline_iqr;
               d["ratio"] = o.decision.ratio;
               d["ratio_iqr"] = o.decision.ratio_iqr;
               d["samples"] = o.decision.rounds;
               d["outer_wgs"] = s.halo_last_outer_wgs(s.time_block());
               // Paired ratios of the per-round maxima over ranks per candidate
               // outer set, and this rank's own ratios (diagnostics).
               py::list rs, ls;
               for (const auto& c : o.ratio_samples) rs.append(py::make_tuple(c.first, c.second));
               for (const auto& c : o.local_ratio_samples) ls.append(py::make_tuple(c.first, c.second));
               d["candidate_ratios"] = rs;
               d["local_candidate_ratios"] = ls;
               d["agreement"] = s.agreement_path();
               d["steady"] = to_string(s.steady_choice());
               d["steady_reason"] = s.steady_reason();
               d["lead_us"] = o.lead_us;
               d["lead_pass_us"] = o.pass_us;
               d["lead_phases_us"] = o.lead_phases;  // (exchange end, inner end, outer end)
               return d;
             });
           },
           "prepare()'s opening decision: the median paired ratio of the per-round maxima over ranks, "
           "interior-first / serial, its IQR, and the medians of the maxima (ms; 0 = not measured)")
      .def("direct_state", [](SolverHandle& h) { return h.visit([](auto& s) { return s.direct_state(); }); },
           "direct halo: '' (not configured), on, pending validation, validated: ..., rejected: ...")
      .def("direct_times",
           [](SolverHandle& h) {
             return h.visit([](auto& s) { return py::make_tuple(s.direct_backend_ms(), s.direct_ms()); });
           },
           "validation timings (ms, worst-rank medians): (backend opening, direct opening); 0 = not measured")
      .def(
          "inject_direct_mismatch",
          [](SolverHandle& h, bool on) { h.visit([on](auto& s) { s.inject_direct_mismatch(on); }); },
          py::arg("on") = true, "fault injection: corrupt one received cell of the direct push before validation")
      .def(
          "inject_direct_skip_wait",
          [](SolverHandle& h, bool on) { h.visit([on](auto& s) { s.inject_direct_skip_wait(on); }); },
          py::arg("on") = true, "fault injection: the validation's direct schedule skips its first wait on this rank")
      .def("agreement_path", [](SolverHandle& h) { return h.visit([](auto& s) { return s.agreement_path(); }); },
           "how collective agreements travel: host allgather, rccl all-reduce or none (one rank)")
      .def("barrier_path", [](SolverHandle& h) { return h.visit([](auto& s) { return s.barrier_path(); }); },
           "the device barrier's path ('' before the first barrier): rccl all-reduce, host allgather (...), "
           "or the host allgather as the agreed fallback after an RCCL barrier failed on some rank")
      .def(
          "set_barrier_comm",
          [](SolverHandle& h, const RcclComm* c) { h.visit([c](auto& s) { s.set_barrier_comm(c); }); },
          py::arg("comm"), py::keep_alive<1, 2>(),
          "tests: the device barrier's own RCCL communicator (default: the halo's)")
      .def(
          "inject_barrier_failure",
          [](SolverHandle& h, bool on) { h.visit([on](auto& s) { s.inject_barrier_failure(on); }); },
          py::arg("on") = true, "fault injection: this rank's RCCL barrier probe fails (tests of the fallback)")
      .def("wire_delay_us", [](SolverHandle& h) { return h.visit([](auto& s) { return s.wire_delay_us(); }); },
           "rehearsal wire time added after each RCCL transfer (us)")
      .def("halo_max_ctas", [](SolverHandle& h) { return h.visit([](auto& s) { return s.halo_max_ctas(); }); },
           "CTA cap of the halo's RCCL communicator (0: RCCL's default)")
      .def("halo_comm_note", [](SolverHandle& h) { return h.visit([](auto& s) { return s.halo_comm_note(); }); })
      .def("abort_halo_comm", [](SolverHandle& h) { h.visit([](auto& s) { s.abort_halo_comm(); }); },
           py::call_guard<py::gil_scoped_release>(),
           "abort the halo's own RCCL communicator (halo_max_ctas), e.g. from a watchdog thread")
      .def("stream_note", [](SolverHandle& h) { return h.visit([](auto& s) { return s.stream_note(); }); },
           "the side stream's hardware-queue check (two-stream schedules)")
      .def("last_run_forks", [](SolverHandle& h) { return h.visit([](auto& s) { return s.last_run_forks(); }); })
      .def("last_run_opening", [](SolverHandle& h) { return h.visit([](auto& s) { return s.last_run_opening(); }); },
           "opening of the last run(): interior-first, serial, fresh, fused, direct, overlap or ''")
      .def(
          "inject_stall",
          [](SolverHandle& h, const std::string& phase, double seconds) {
            h.visit([&](auto& s) { s.inject_stall(phase, seconds); });
          },
          py::arg("phase"), py::arg("seconds"),
          "fault injection: sleep `seconds` on entering `phase` (prepare, warm, run, profile_window)")
      .def(
          "profile_window",
          [](SolverHandle& h, int iters) {
            WindowPhases w;
            {
              py::gil_scoped_release nogil;
              w = h.visit([iters](auto& s) { return s.profile_window(iters); });
            }
            py::dict d;
            d["opening"] = w.opening;
            d["exchanges"] = w.exchanges;
            d["host_enqueue_us"] = w.host_enqueue_us;
            d["gpu_span_us"] = w.gpu_span_us;
            d["wall_us"] = w.wall_us;
            d["plain_wall_us"] = w.plain_wall_us;
            py::list ph;
            for (const auto& [name, t0, t1] : w.phases) ph.append(py::make_tuple(name, t0, t1));
            d["phases"] = ph;
            return d;
          },
          py::arg("iters"),
          "collective, state-preserving: one event-timed replica of run(iters)'s opening super-step "
          "(phases: (stream:phase, start us, end us))")
      .def("sum_form_active", [](SolverHandle& h) { return h.visit([](auto& s) { return s.sum_form_active(); }); })
      .def("scaled_form_active",
           [](SolverHandle& h) { return h.visit([](auto& s) { return s.scaled_form_active(); }); })
      .def("sum_form_note", [](SolverHandle& h) { return h.visit([](auto& s) { return s.sum_form_note(); }); })
      .def("relaxation_note", [](SolverHandle& h) { return h.visit([](auto& s) { return s.relaxation_note(); }); },
           "the relaxation cycle: which passes run and why, with M, the weights' range and growth ('' without one)")
      .def("relaxation_info",
           [](SolverHandle& h) {
             return h.visit([](auto& s) {
               py::dict d;
               const kernels::LevelTable& t = s.relaxation_table();
               d["cycle"] = s.relaxation_cycle();
               d["active"] = s.relaxation_active();
               d["omega_min"] = s.relaxation_omega_min();
               d["omega_max"] = s.relaxation_omega_max();
               d["growth"] = s.relaxation_growth();
               d["center"] = std::vector<double>(t.center, t.center + t.n);
               d["neighbor"] = std::vector<double>(t.neighbor, t.neighbor + t.n);
               return d;
             });
           },
           "the agreed relaxation cycle: cycle (levels, 0 without one), active (the level passes run), omega_min, "
           "omega_max, growth and the per-level (center, neighbor) coefficients")
      .def("last_run_blocks", [](SolverHandle& h) { return h.visit([](auto& s) { return s.last_run_blocks(); }); },
           "(S, count) super-steps the last run() enqueued")
      .def("last_run_exchanges", [](SolverHandle& h) { return h.visit([](auto& s) { return s.last_run_exchanges(); }); },
           "halo exchanges the last run() enqueued (priming included)")
      .def("step", [](SolverHandle& h) { h.visit([](auto& s) { s.step(); }); })
      .def("direct_halo", [](SolverHandle& h) { return h.visit([](auto& s) { return s.direct_halo(); }); },
           "whether halos are pushed tile-to-tile by the device (IPC backend, direct mode)")
      .def("graph_supersteps", [](SolverHandle& h) { return h.visit([](auto& s) { return s.graph_supersteps(); }); })
      .def(
          "run", [](SolverHandle& h, int n) { h.visit([n](auto& s) { s.run(n); }); }, py::arg("iters"),
          py::call_guard<py::gil_scoped_release>())
      .def(
          "prepare", [](SolverHandle& h, int n) { h.visit([n](auto& s) { s.prepare(n); }); }, py::arg("iters"),
          py::call_guard<py::gil_scoped_release>(),
          "capture graphs and launch every kernel shape run(iters) uses, without advancing the state")
      .def(
          "warm", [](SolverHandle& h, int n, int passes) { h.visit([n, passes](auto& s) { s.warm(n, passes); }); },
          py::arg("iters"), py::arg("passes"), py::call_guard<py::gil_scoped_release>(),
          "untimed state-preserving passes of run(iters)'s shapes (sustained clocks before a short window)")
      .def("exchange_only", [](SolverHandle& h) { h.visit([](auto& s) { s.exchange_only(); }); })
      .def(
          "residual",
          [](SolverHandle& h) {
            Residual r;
            {
              py::gil_scoped_release nogil;
              r = h.visit([](auto& s) { return s.residual(); });
            }
            py::dict d;
            d["linf"] = r.linf;
            d["l2"] = r.l2;
            d["cells"] = r.cells;
            return d;
          },
          "collective: norms of the Jacobi residual r = A u - u over the global core (the change the next "
          "single step would make), agreed over ranks; the field is unchanged")
      .def(
          "run_until",
          [](SolverHandle& h, double tol, int max_iters, int check_every, const std::string& norm) {
            if (norm != "linf" && norm != "l2") throw std::invalid_argument("norm must be linf or l2, got '" + norm + "'");
            const Norm n = norm == "l2" ? Norm::L2 : Norm::Linf;
            RunUntil r;
            {
              py::gil_scoped_release nogil;
              r = h.visit([&](auto& s) { return s.run_until(tol, max_iters, check_every, n); });
            }
            py::dict d;
            d["converged"] = r.converged;
            d["iterations"] = r.iterations;
            d["residual"] = r.residual;
            d["checks"] = r.checks;
            d["check_every"] = r.check_every;
            d["max_iters"] = r.max_iters;
            d["reason"] = r.reason;
            d["norm"] = norm;
            py::list hist;
            for (const auto& [it, linf, l2] : r.history) hist.append(py::make_tuple(it, linf, l2));
            d["history"] = hist;
            return d;
          },
          py::arg("tol"), py::arg("max_iters"), py::arg("check_every") = 0, py::arg("norm") = "linf",
          "collective: run(check_every) + residual() until the agreed norm is <= tol, max_iters iterations ran or "
          "the norm is not finite (check_every = 0: DEFAULT_CHECK_BLOCKS x time_block)")
      .def("synchronize", [](SolverHandle& h) { h.visit([](auto& s) { s.synchronize(); }); },
           py::call_guard<py::gil_scoped_release>())
      .def("current",
           [](SolverHandle& h) {
             return h.visit([](auto& s) { return reinterpret_cast<std::uintptr_t>(s.current()); });
           })
      .def("main_stream",
           [](SolverHandle& h) {
             return h.visit([](auto& s) { return reinterpret_cast<std::uintptr_t>(s.main_stream()); });
           })
      .def("side_stream",
           [](SolverHandle& h) {
             return h.visit([](auto& s) { return reinterpret_cast<std::uintptr_t>(s.side_stream()); });
           })
      .def("graph_active", [](SolverHandle& h) { return h.visit([](auto& s) { return s.graph_active(); }); })
      .def("graph_status", [](SolverHandle& h) { return h.visit([](auto& s) { return s.graph_status(); }); })
      .def("fused_periodic", [](SolverHandle& h) { return h.visit([](auto& s) { return s.fused_periodic(); }); })
      .def("overlapped", [](SolverHandle& h) { return h.visit([](auto& s) { return s.overlapped(); }); })
      .def("time_block", [](SolverHandle& h) { return h.visit([](auto& s) { return s.time_block(); }); });

  // ------------------------------------------------------------------ multigrid
  auto sweep_table = [](const std::vector<double>& center, const std::vector<double>& neighbor,
                        const std::vector<double>& weight) {
    if (center.size() != neighbor.size() || center.size() != weight.size() || center.empty() ||
        int(center.size()) > kernels::kMaxLevels)
      throw std::invalid_argument("a sweep table takes 1.." + std::to_string(kernels::kMaxLevels) +
                                  " (center, neighbor, weight) triples");
    kernels::MgSweepTable t;
    t.n = int(center.size());
    for (int l = 0; l < t.n; ++l) {
      t.center[l] = center[size_t(l)];
      t.neighbor[l] = neighbor[size_t(l)];
      t.weight[l] = weight[size_t(l)];
    }
    return t;
  };
  m.def(
      "mg_smooth",
      [sweep_table](std::uintptr_t in, std::uintptr_t out, std::uintptr_t src, const TileGeom& g,
                    const std::vector<double>& center, const std::vector<double>& neighbor,
                    const std::vector<double>& weight, const std::string& dt, std::uintptr_t s) {
        const kernels::MgSweepTable t = sweep_table(center, neighbor, weight);
        if (parse_dtype(dt) == DType::F32)
          kernels::mg_smooth<float>(ptr<float>(in), ptr<float>(out), ptr<float>(src), g, t, strm(s));
        else
          kernels::mg_smooth<double>(ptr<double>(in), ptr<double>(out), ptr<double>(src), g, t, strm(s));
      },
      py::arg("u_in"), py::arg("u_out"), py::arg("src"), py::arg("geom"), py::arg("center"), py::arg("neighbor"),
      py::arg("weight"), py::arg("dtype") = "f32", py::arg("stream") = 0,
      "len(center) (1..4) fused sweeps x' = fma(neighbor[l], (n + s) + (w + e), center[l] * c) + T(weight[l]) * g over "
      "the core of a ring-1 tile, ring cells held; writes the core of u_out only");
  m.def(
      "mg_residual_restrict",
      [](std::uintptr_t u, std::uintptr_t src, const TileGeom& g, std::uintptr_t csrc, const TileGeom& gc, double c0,
         double c1, const std::string& dt, std::uintptr_t s) {
        kernels::Stencil5Coeffs c{c0, c1, false, -1.0};
        if (parse_dtype(dt) == DType::F32)
          kernels::mg_residual_restrict<float>(ptr<float>(u), ptr<float>(src), g, ptr<float>(csrc), gc, c, strm(s));
        else
          kernels::mg_residual_restrict<double>(ptr<double>(u), ptr<double>(src), g, ptr<double>(csrc), gc, c, strm(s));
      },
      py::arg("u"), py::arg("src"), py::arg("geom"), py::arg("coarse_src"), py::arg("coarse_geom"),
      py::arg("c_center") = 0.2, py::arg("c_neighbor") = 0.2, py::arg("dtype") = "f32", py::arg("stream") = 0,
      "coarse_src core = 4 R ((A u + src) - u): the fine residual and full weighting fused, no fine residual array");
  m.def(
      "mg_prolong_add",
      [](std::uintptr_t e, const TileGeom& gc, std::uintptr_t u, const TileGeom& g, const std::string& dt,
         std::uintptr_t s) {
        if (parse_dtype(dt) == DType::F32) kernels::mg_prolong_add<float>(ptr<float>(e), gc, ptr<float>(u), g, strm(s));
        else kernels::mg_prolong_add<double>(ptr<double>(e), gc, ptr<double>(u), g, strm(s));
      },
      py::arg("e"), py::arg("coarse_geom"), py::arg("u"), py::arg("geom"), py::arg("dtype") = "f32",
      py::arg("stream") = 0, "u core += P e (bilinear, e = 0 outside the coarse core), in place");
  m.def(
      "mg_coarse_solve",
      [sweep_table](std::uintptr_t src, std::uintptr_t e, const TileGeom& g, const std::vector<double>& center,
                    const std::vector<double>& neighbor, const std::vector<double>& weight, int repeats,
                    const std::string& dt, std::uintptr_t s) {
        const kernels::MgSweepTable t = sweep_table(center, neighbor, weight);
        if (parse_dtype(dt) == DType::F32)
          kernels::mg_coarse_solve<float>(ptr<float>(src), ptr<float>(e), g, t, repeats, strm(s));
        else
          kernels::mg_coarse_solve<double>(ptr<double>(src), ptr<double>(e), g, t, repeats, strm(s));
      },
      py::arg("src"), py::arg("e"), py::arg("geom"), py::arg("center"), py::arg("neighbor"), py::arg("weight"),
      py::arg("repeats"), py::arg("dtype") = "f32", py::arg("stream") = 0,
      "repeats x len(center) sweeps from e = 0 on a grid of at most 63 x 63 in one workgroup's LDS; writes the core of e");
  m.def("last_multigrid_dispatch", [] { return std::string(kernels::last_multigrid_dispatch()); },
        "the kernel the most recent multigrid launcher ran ('' before the first)");

  py::class_<MultigridHandle> multigrid_solver(m, "MultigridSolver");
  multigrid_solver
      .def(py::init([](index_t w, index_t h, const std::string& dt, double c0, double c1, int nu_pre, int nu_post,
                       double omega, double coarse_reduction, bool graph) {
             MultigridConfig cfg;
             cfg.width = w;
             cfg.height = h;
             cfg.c_center = c0;
             cfg.c_neighbor = c1;
             cfg.nu_pre = nu_pre;
             cfg.nu_post = nu_post;
             cfg.smoother_omega = omega;
             cfg.coarse_reduction = coarse_reduction;
             cfg.graph = graph;
             return MultigridHandle::make(dt, cfg);
           }),
           py::arg("width"), py::arg("height"), py::arg("dtype") = "f64", py::arg("c_center") = 0.2,
           py::arg("c_neighbor") = 0.2, py::arg("nu_pre") = 2, py::arg("nu_post") = 2, py::arg("smoother_omega") = 0.8,
           py::arg("coarse_reduction") = 1e-3, py::arg("graph") = true)
      .def("levels",
           [](MultigridHandle& h) {
             std::vector<std::pair<long long, long long>> out;
             h.visit([&](auto& s) {
               for (const auto& l : s.levels()) out.emplace_back(l.width, l.height);
             });
             return out;
           })
      .def("vcycle", [](MultigridHandle& h, int n) { h.visit([&](auto& s) { s.vcycle(n); }); }, py::arg("n") = 1,
           py::call_guard<py::gil_scoped_release>())
      .def(
          "solve",
          [](MultigridHandle& h, double tol, int max_cycles, const std::string& norm) {
            MultigridSolve r;
            {
              py::gil_scoped_release nogil;
              r = h.visit([&](auto& s) { return s.solve(tol, max_cycles, norm); });
            }
            py::dict d;
            d["converged"] = r.converged;
            d["cycles"] = r.cycles;
            d["residual"] = r.residual;
            d["reason"] = r.reason;
            d["norm"] = r.norm;
            py::list hist;
            for (const auto& c : r.history) hist.append(py::make_tuple(c.cycle, c.linf, c.l2));
            d["history"] = hist;
            return d;
          },
          py::arg("tol"), py::arg("max_cycles") = 50, py::arg("norm") = "l2",
          "residual() + vcycle(1) until the norm is <= tol, max_cycles ran, the norm is not finite, or no new best "
          "residual for 3 consecutive cycles ('stalled')")
      .def("launches_per_cycle", [](MultigridHandle& h) { return h.visit([](auto& s) { return s.launches_per_cycle(); }); });
  def_poisson_methods(multigrid_solver);

  // ------------------------------------------------------- conjugate gradients
  // The launchers take the scalar block (CG_SCALARS_BYTES: doubles rr, pq, alpha,
  // beta, linf, tol, then ints iteration, max_iters, norm, status), the partials
  // (2 * cg_grid_size(geom) doubles) and the ticket (one unsigned, 0 before the
  // first launch) as device addresses.
  m.attr("CG_SCALARS_BYTES") = int(sizeof(kernels::CgScalars));
  m.def("cg_grid_size", &kernels::cg_grid_size, py::arg("geom"), "workgroups of a CG launch at most (either type)");
  m.def(
      "cg_start",
      [](std::uintptr_t u, std::uintptr_t g, std::uintptr_t r, std::uintptr_t p, const TileGeom& geom, double c0,
         double c1, std::uintptr_t scalars, std::uintptr_t partials, std::uintptr_t counter, const std::string& dt,
         std::uintptr_t s, const std::array<int, 4>& sides) {
        kernels::Stencil5Coeffs c{c0, c1, false, -1.0};
        if (parse_dtype(dt) == DType::F32)
          kernels::cg_start<float>(ptr<float>(u), ptr<float>(g), ptr<float>(r), ptr<float>(p), geom, c,
                                   ptr<kernels::CgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s), ghost_sides(sides));
        else
          kernels::cg_start<double>(ptr<double>(u), ptr<double>(g), ptr<double>(r), ptr<double>(p), geom, c,
                                    ptr<kernels::CgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s), ghost_sides(sides));
      },
      py::arg("u"), py::arg("g"), py::arg("r"), py::arg("p"), py::arg("geom"), py::arg("c_center"), py::arg("c_neighbor"),
      py::arg("scalars"), py::arg("partials"), py::arg("counter"), py::arg("dtype") = "f64", py::arg("stream") = 0, py::arg("sides") = kNoSides,
      "r = p = (fma(c1, (n + s) + (w + e), c0 v) + g) - v over the core; last workgroup: rr, linf, beta = 0, "
      "iteration = 0, status");
  m.def(
      "cg_heat_start",
      [](std::uintptr_t u, std::uintptr_t q, std::uintptr_t g, std::uintptr_t r, std::uintptr_t p, const TileGeom& geom,
         double lam, double theta, std::uintptr_t scalars, std::uintptr_t partials, std::uintptr_t counter,
         const std::string& dt, std::uintptr_t s, const std::array<int, 4>& sides) {
        const kernels::HeatCoeffs hc = kernels::heat_coefficients(lam, theta);
        if (parse_dtype(dt) == DType::F32)
          kernels::cg_heat_start<float>(ptr<float>(u), ptr<float>(q), ptr<float>(g), ptr<float>(r), ptr<float>(p), geom, hc,
                                        ptr<kernels::CgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s), ghost_sides(sides));
        else
          kernels::cg_heat_start<double>(ptr<double>(u), ptr<double>(q), ptr<double>(g), ptr<double>(r), ptr<double>(p), geom, hc,
                                         ptr<kernels::CgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s), ghost_sides(sides));
      },
      py::arg("u"), py::arg("q"), py::arg("g"), py::arg("r"), py::arg("p"), py::arg("geom"), py::arg("lam"),
      py::arg("theta"), py::arg("scalars"), py::arg("partials"), py::arg("counter"), py::arg("dtype") = "f64",
      py::arg("stream") = 0, py::arg("sides") = kNoSides,
      "the start of an implicit heat step: g = fma(b, S, a v) (+ s q; q = 0: no source), r = p = (fma(c1, S, 0 v) + g) "
      "- v over the core with S = (n + s) + (w + e); last workgroup: as cg_start");
  m.def(
      "cg_apply",
      [](std::uintptr_t r, std::uintptr_t p_old, std::uintptr_t p_new, std::uintptr_t q, const TileGeom& geom, double c0,
         double c1, std::uintptr_t scalars, std::uintptr_t partials, std::uintptr_t counter, const std::string& dt,
         std::uintptr_t s, const std::array<int, 4>& sides) {
        kernels::Stencil5Coeffs c{c0, c1, false, -1.0};
        if (parse_dtype(dt) == DType::F32)
          kernels::cg_apply<float>(ptr<float>(r), ptr<float>(p_old), ptr<float>(p_new), ptr<float>(q), geom, c,
                                   ptr<kernels::CgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s), ghost_sides(sides));
        else
          kernels::cg_apply<double>(ptr<double>(r), ptr<double>(p_old), ptr<double>(p_new), ptr<double>(q), geom, c,
                                    ptr<kernels::CgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s), ghost_sides(sides));
      },
      py::arg("r"), py::arg("p_old"), py::arg("p_new"), py::arg("q"), py::arg("geom"), py::arg("c_center"),
      py::arg("c_neighbor"), py::arg("scalars"), py::arg("partials"), py::arg("counter"), py::arg("dtype") = "f64",
      py::arg("stream") = 0, py::arg("sides") = kNoSides,
      "p_new = fma(T(beta), p_old, r), q = fma(-c1, (n + s) + (w + e), T(1 - c0) p_new) with p_new = 0 outside the "
      "core; last workgroup: pq, alpha (or status 3)");
  m.def(
      "cg_update",
      [](std::uintptr_t u, std::uintptr_t r, std::uintptr_t p, std::uintptr_t q, const TileGeom& geom,
         std::uintptr_t scalars, std::uintptr_t partials, std::uintptr_t counter, const std::string& dt, std::uintptr_t s) {
        if (parse_dtype(dt) == DType::F32)
          kernels::cg_update<float>(ptr<float>(u), ptr<float>(r), ptr<float>(p), ptr<float>(q), geom,
                                    ptr<kernels::CgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s));
        else
          kernels::cg_update<double>(ptr<double>(u), ptr<double>(r), ptr<double>(p), ptr<double>(q), geom,
                                     ptr<kernels::CgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s));
      },
      py::arg("u"), py::arg("r"), py::arg("p"), py::arg("q"), py::arg("geom"), py::arg("scalars"), py::arg("partials"),
      py::arg("counter"), py::arg("dtype") = "f64", py::arg("stream") = 0,
      "u = fma(T(alpha), p, u), r = fma(-T(alpha), q, r) in place; last workgroup: rr, linf, beta, ++iteration, status");
  m.def("last_cg_dispatch", [] { return std::string(kernels::last_cg_dispatch()); },
        "the kernel the most recent CG launcher ran ('' before the first)");

  py::class_<CgHandle> cg_solver(m, "CgSolver");
  cg_solver.def(py::init([](index_t w, index_t h, const std::string& dt, double c0, double c1, bool graph,
                            const std::vector<std::string>& neumann) {
                  CgConfig cfg;
                  cfg.neumann = neumann;
                  cfg.width = w;
                  cfg.height = h;
                  cfg.c_center = c0;
                  cfg.c_neighbor = c1;
                  cfg.graph = graph;
                  return CgHandle::make(dt, cfg);
                }),
                py::arg("width"), py::arg("height"), py::arg("dtype") = "f64", py::arg("c_center") = 0.2,
                py::arg("c_neighbor") = 0.2, py::arg("graph") = true, py::arg("neumann") = std::vector<std::string>{});
  def_poisson_methods(cg_solver);
  def_cg_methods(cg_solver, 10000, 32,
                 "cg_start, then blocks of check_every iterations and a read of the device scalars until the device "
                 "stops; a reported convergence is confirmed on the true residual (else a restart, 'stalled' after 3)");

  // ---------------------------------------------------------- preconditioned CG
  // The scalar block is PCG_SCALARS_BYTES: doubles rr, rz, pq, alpha, beta, linf,
  // tol, then ints iteration, max_iters, norm, status. Partials: 2 *
  // cg_grid_size(geom) doubles for pcg_*, 2 * mgp_smooth_grid_size(geom) for the
  // smoother's dot epilogue; the ticket is CG's.
  m.attr("PCG_SCALARS_BYTES") = int(sizeof(kernels::PcgScalars));
  m.def("mgp_smooth_grid_size", &kernels::mgp_smooth_grid_size, py::arg("geom"), "workgroups of an mgp_smooth launch");
  m.def(
      "pcg_start",
      [](std::uintptr_t u, std::uintptr_t g, std::uintptr_t r, const TileGeom& geom, double c0, double c1,
         std::uintptr_t scalars, std::uintptr_t partials, std::uintptr_t counter, const std::string& dt, std::uintptr_t s, const std::array<int, 4>& sides) {
        kernels::Stencil5Coeffs c{c0, c1, false, -1.0};
        if (parse_dtype(dt) == DType::F32)
          kernels::pcg_start<float>(ptr<float>(u), ptr<float>(g), ptr<float>(r), geom, c,
                                    ptr<kernels::PcgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s), ghost_sides(sides));
        else
          kernels::pcg_start<double>(ptr<double>(u), ptr<double>(g), ptr<double>(r), geom, c,
                                     ptr<kernels::PcgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s), ghost_sides(sides));
      },
      py::arg("u"), py::arg("g"), py::arg("r"), py::arg("geom"), py::arg("c_center"), py::arg("c_neighbor"),
      py::arg("scalars"), py::arg("partials"), py::arg("counter"), py::arg("dtype") = "f64", py::arg("stream") = 0, py::arg("sides") = kNoSides,
      "r = (fma(c1, (n + s) + (w + e), c0 v) + g) - v over the core; last workgroup: rr, linf, rz = beta = 0, "
      "iteration = 0, status");
  m.def(
      "pcg_heat_start",
      [](std::uintptr_t u, std::uintptr_t q, std::uintptr_t g, std::uintptr_t r, const TileGeom& geom, double lam,
         double theta, std::uintptr_t scalars, std::uintptr_t partials, std::uintptr_t counter, const std::string& dt,
         std::uintptr_t s, const std::array<int, 4>& sides) {
        const kernels::HeatCoeffs hc = kernels::heat_coefficients(lam, theta);
        if (parse_dtype(dt) == DType::F32)
          kernels::pcg_heat_start<float>(ptr<float>(u), ptr<float>(q), ptr<float>(g), ptr<float>(r), geom, hc,
                                         ptr<kernels::PcgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s), ghost_sides(sides));
        else
          kernels::pcg_heat_start<double>(ptr<double>(u), ptr<double>(q), ptr<double>(g), ptr<double>(r), geom, hc,
                                          ptr<kernels::PcgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s), ghost_sides(sides));
      },
      py::arg("u"), py::arg("q"), py::arg("g"), py::arg("r"), py::arg("geom"), py::arg("lam"), py::arg("theta"),
      py::arg("scalars"), py::arg("partials"), py::arg("counter"), py::arg("dtype") = "f64", py::arg("stream") = 0,
      py::arg("sides") = kNoSides,
      "cg_heat_start on a PcgScalars block: g and r over the core, no first direction; last workgroup: as pcg_start");
  m.def(
      "pcg_apply",
      [](std::uintptr_t z, std::uintptr_t p_old, std::uintptr_t p_new, std::uintptr_t q, const TileGeom& geom, double c0,
         double c1, std::uintptr_t scalars, std::uintptr_t partials, std::uintptr_t counter, const std::string& dt,
         std::uintptr_t s, const std::array<int, 4>& sides) {
        kernels::Stencil5Coeffs c{c0, c1, false, -1.0};
        if (parse_dtype(dt) == DType::F32)
          kernels::pcg_apply<float>(ptr<float>(z), ptr<float>(p_old), ptr<float>(p_new), ptr<float>(q), geom, c,
                                    ptr<kernels::PcgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s), ghost_sides(sides));
        else
          kernels::pcg_apply<double>(ptr<double>(z), ptr<double>(p_old), ptr<double>(p_new), ptr<double>(q), geom, c,
                                     ptr<kernels::PcgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s), ghost_sides(sides));
      },
      py::arg("z"), py::arg("p_old"), py::arg("p_new"), py::arg("q"), py::arg("geom"), py::arg("c_center"),
      py::arg("c_neighbor"), py::arg("scalars"), py::arg("partials"), py::arg("counter"), py::arg("dtype") = "f64",
      py::arg("stream") = 0, py::arg("sides") = kNoSides,
      "p_new = fma(T(beta), p_old, z), q = L p_new; last workgroup: pq, alpha = rz / pq (or status 3)");
  m.def(
      "pcg_update",
      [](std::uintptr_t u, std::uintptr_t r, std::uintptr_t p, std::uintptr_t q, const TileGeom& geom,
         std::uintptr_t scalars, std::uintptr_t partials, std::uintptr_t counter, const std::string& dt, std::uintptr_t s) {
        if (parse_dtype(dt) == DType::F32)
          kernels::pcg_update<float>(ptr<float>(u), ptr<float>(r), ptr<float>(p), ptr<float>(q), geom,
                                     ptr<kernels::PcgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s));
        else
          kernels::pcg_update<double>(ptr<double>(u), ptr<double>(r), ptr<double>(p), ptr<double>(q), geom,
                                      ptr<kernels::PcgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s));
      },
      py::arg("u"), py::arg("r"), py::arg("p"), py::arg("q"), py::arg("geom"), py::arg("scalars"), py::arg("partials"),
      py::arg("counter"), py::arg("dtype") = "f64", py::arg("stream") = 0,
      "u = fma(T(alpha), p, u), r = fma(-T(alpha), q, r) in place; last workgroup: rr, linf, ++iteration, status");
  m.def(
      "mgp_smooth",
      [sweep_table](std::uintptr_t in, std::uintptr_t out, std::uintptr_t src, const TileGeom& g,
                    const std::vector<double>& center, const std::vector<double>& neighbor,
                    const std::vector<double>& weight, bool rr, bool rc, std::uintptr_t scalars, std::uintptr_t partials,
                    std::uintptr_t counter, const std::string& dt, std::uintptr_t s, const std::array<int, 4>& sides) {
        const kernels::GhostSides sd = ghost_sides(sides, rr, rc);
        const kernels::MgSweepTable t = sweep_table(center, neighbor, weight);
        if (parse_dtype(dt) == DType::F32)
          kernels::mgp_smooth<float>(ptr<float>(in), ptr<float>(out), ptr<float>(src), g, t, sd,
                                     ptr<kernels::PcgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s));
        else
          kernels::mgp_smooth<double>(ptr<double>(in), ptr<double>(out), ptr<double>(src), g, t, sd,
                                      ptr<kernels::PcgScalars>(scalars), ptr<double>(partials), ptr<unsigned>(counter), strm(s));
      },
      py::arg("u_in"), py::arg("u_out"), py::arg("src"), py::arg("geom"), py::arg("center"), py::arg("neighbor"),
      py::arg("weight"), py::arg("reflect_rows") = false, py::arg("reflect_cols") = false, py::arg("scalars") = 0,
      py::arg("partials") = 0, py::arg("counter") = 0, py::arg("dtype") = "f32", py::arg("stream") = 0, py::arg("sides") = kNoSides,
      "mg_smooth with reflecting ghosts; with scalars, partials and counter also the dot epilogue (rz, beta)");
  m.def(
      "mgp_residual_restrict",
      [](std::uintptr_t u, std::uintptr_t src, const TileGeom& g, bool rr, bool rc, std::uintptr_t csrc, const TileGeom& gc,
         double c0, double c1, const std::string& dt, std::uintptr_t s, const std::array<int, 4>& sides) {
        const kernels::GhostSides sd = ghost_sides(sides, rr, rc);
        kernels::Stencil5Coeffs c{c0, c1, false, -1.0};
        if (parse_dtype(dt) == DType::F32)
          kernels::mgp_residual_restrict<float>(ptr<float>(u), ptr<float>(src), g, sd, ptr<float>(csrc), gc, c, strm(s));
        else
          kernels::mgp_residual_restrict<double>(ptr<double>(u), ptr<double>(src), g, sd, ptr<double>(csrc), gc, c,
                                                 strm(s));
      },
      py::arg("u"), py::arg("src"), py::arg("geom"), py::arg("reflect_rows"), py::arg("reflect_cols"),
      py::arg("coarse_src"), py::arg("coarse_geom"), py::arg("c_center") = 0.2, py::arg("c_neighbor") = 0.2,
      py::arg("dtype") = "f32", py::arg("stream") = 0, py::arg("sides") = kNoSides,
      "coarse_src core = 4 R ((A u + src) - u) for a coarse tile of (width / 2) x (height / 2), fine residuals outside "
      "the core 0, the fine level's reflecting ghost read");
  m.def(
      "mgp_prolong_add",
      [](std::uintptr_t e, const TileGeom& gc, std::uintptr_t u, const TileGeom& g, const std::string& dt,
         std::uintptr_t s, const std::array<int, 4>& sides) {
        if (parse_dtype(dt) == DType::F32) kernels::mgp_prolong_add<float>(ptr<float>(e), gc, ptr<float>(u), g, strm(s), ghost_sides(sides));
        else kernels::mgp_prolong_add<double>(ptr<double>(e), gc, ptr<double>(u), g, strm(s), ghost_sides(sides));
      },
      py::arg("e"), py::arg("coarse_geom"), py::arg("u"), py::arg("geom"), py::arg("dtype") = "f32",
      py::arg("stream") = 0, py::arg("sides") = kNoSides, "u core += P e for a coarse tile of (width / 2) x (height / 2)");
  m.def(
      "mgp_coarse_solve",
      [sweep_table](std::uintptr_t src, std::uintptr_t e, const TileGeom& g, const std::vector<double>& center,
                    const std::vector<double>& neighbor, const std::vector<double>& weight, int repeats, bool rr, bool rc,
                    std::uintptr_t scalars, const std::string& dt, std::uintptr_t s, const std::array<int, 4>& sides) {
        const kernels::GhostSides sd = ghost_sides(sides, rr, rc);
        const kernels::MgSweepTable t = sweep_table(center, neighbor, weight);
        if (parse_dtype(dt) == DType::F32)
          kernels::mgp_coarse_solve<float>(ptr<float>(src), ptr<float>(e), g, t, repeats, sd,
                                           ptr<kernels::PcgScalars>(scalars), strm(s));
        else
          kernels::mgp_coarse_solve<double>(ptr<double>(src), ptr<double>(e), g, t, repeats, sd,
                                            ptr<kernels::PcgScalars>(scalars), strm(s));
      },
      py::arg("src"), py::arg("e"), py::arg("geom"), py::arg("center"), py::arg("neighbor"), py::arg("weight"),
      py::arg("repeats"), py::arg("reflect_rows") = false, py::arg("reflect_cols") = false, py::arg("scalars") = 0,
      py::arg("dtype") = "f32", py::arg("stream") = 0, py::arg("sides") = kNoSides,
      "mg_coarse_solve with reflecting ghosts; with scalars also the dot epilogue of a single-level preconditioner");
  m.def("last_pcg_dispatch", [] { return std::string(kernels::last_pcg_dispatch()); },
        "the kernel the most recent preconditioner launcher ran ('' before the first)");

  py::class_<PcgHandle> pcg_solver(m, "PcgSolver");
  pcg_solver
      .def(py::init([](index_t w, index_t h, const std::string& dt, double c0, double c1, int nu, double omega,
                       double coarse_reduction, bool graph, const std::vector<std::string>& neumann) {
             PcgConfig cfg;
             cfg.neumann = neumann;
             cfg.width = w;
             cfg.height = h;
             cfg.c_center = c0;
             cfg.c_neighbor = c1;
             cfg.nu = nu;
             cfg.smoother_omega = omega;
             cfg.coarse_reduction = coarse_reduction;
             cfg.graph = graph;
             return PcgHandle::make(dt, cfg);
           }),
           py::arg("width"), py::arg("height"), py::arg("dtype") = "f64", py::arg("c_center") = 0.2,
           py::arg("c_neighbor") = 0.2, py::arg("nu") = 2, py::arg("smoother_omega") = 0.8,
           py::arg("coarse_reduction") = 1e-3, py::arg("graph") = true,
           py::arg("neumann") = std::vector<std::string>{})
      .def("levels",
           [](PcgHandle& h) {
             py::list out;
             h.visit([&](auto& s) {
               for (const auto& l : s.levels())
                 out.append(py::make_tuple(l.width, l.height, l.reflect_rows, l.reflect_cols, l.c0));  // codes: pcg_plan_levels
             });
             return out;
           })
      .def("launches_per_iteration", [](PcgHandle& h) { return h.visit([](auto& s) { return s.launches_per_iteration(); }); });
  def_poisson_methods(pcg_solver);
  def_cg_methods(pcg_solver, 1000, 2,
                 "pcg_start, then blocks of check_every iterations (V-cycle, pcg_apply, pcg_update) and a read of the "
                 "device scalars until the device stops; a reported convergence is confirmed on the true residual");

  // ------------------------------------------------------------------ ping-pong
  py::enum_<PingPongMode>(m, "PingPongMode")
      .value("BLOCKING", PingPongMode::Blocking)
      .value("ASYNC", PingPongMode::Async)
      .value("OVERLAP", PingPongMode::Overlap)
      .value("BIDIRECTIONAL", PingPongMode::Bidirectional);
  py::enum_<LocalPath>(m, "LocalPath")
      .value("DEVICE_COPY", LocalPath::DeviceCopy)
      .value("PINNED_STAGING", LocalPath::PinnedStaging)
      .value("PAGEABLE_STAGING", LocalPath::PageableStaging);
  py::class_<PingPongStats>(m, "PingPongStats")
      .def_readonly("bytes", &PingPongStats::bytes)
      .def_readonly("reps", &PingPongStats::reps)
      .def_readonly("min_rtt_us", &PingPongStats::min_rtt_us)
      .def_readonly("median_rtt_us", &PingPongStats::median_rtt_us)
      .def_readonly("max_rtt_us", &PingPongStats::max_rtt_us)
      .def_readonly("compute_alone_us", &PingPongStats::compute_alone_us)
      .def_readonly("comm_alone_us", &PingPongStats::comm_alone_us)
      .def_readonly("overlapped_us", &PingPongStats::overlapped_us)
      .def_readonly("verified", &PingPongStats::verified)
      .def("latency_us", &PingPongStats::latency_us)
      .def("bandwidth_gbps", &PingPongStats::bandwidth_gbps)
      .def("bidir_gbps", &PingPongStats::bidir_gbps);
  m.def(
      "pingpong_rccl",
      [](const RcclComm& c, int peer, std::uintptr_t sb, std::uintptr_t rb, size_t bytes, int warmup, int reps,
         PingPongMode mode, std::uintptr_t s) {
        return pingpong_rccl(c, peer, ptr<void>(sb), ptr<void>(rb), bytes, warmup, reps, mode, strm(s));
      },
      py::arg("comm"), py::arg("peer"), py::arg("sendbuf"), py::arg("recvbuf"), py::arg("nbytes"),
      py::arg("warmup") = 5, py::arg("reps") = 20, py::arg("mode") = PingPongMode::Blocking, py::arg("stream") = 0,
      py::call_guard<py::gil_scoped_release>());
  m.def(
      "pingpong_local",
      [](LocalPath p, std::uintptr_t a, std::uintptr_t b, size_t bytes, int warmup, int reps, std::uintptr_t s) {
        return pingpong_local(p, ptr<void>(a), ptr<void>(b), bytes, warmup, reps, strm(s));
      },
      py::arg("path"), py::arg("buf_a"), py::arg("buf_b"), py::arg("nbytes"), py::arg("warmup") = 5,
      py::arg("reps") = 20, py::arg("stream") = 0, py::call_guard<py::gil_scoped_release>());

  // Device-initiated ping-pong over HIP IPC mappings (runtime/ipc.hpp).
  py::class_<IpcMailbox>(m, "IpcMailbox")
      .def(py::init<size_t>(), py::arg("capacity"))
      .def("handle", [](const IpcMailbox& b) { return py::bytes(b.handle()); })
      .def("base", [](const IpcMailbox& b) { return reinterpret_cast<std::uintptr_t>(b.base()); })
      .def("data", [](const IpcMailbox& b) { return reinterpret_cast<std::uintptr_t>(b.data()); })
      .def_property_readonly("capacity", &IpcMailbox::capacity);
  py::class_<IpcPeerMailbox>(m, "IpcPeerMailbox")
      .def(py::init([](py::bytes h) { return new IpcPeerMailbox(std::string(h)); }), py::arg("handle"))
      .def("base", [](const IpcPeerMailbox& b) { return reinterpret_cast<std::uintptr_t>(b.base()); });
  m.def(
      "pingpong_ipc",
      [](const IpcMailbox& mine, std::uintptr_t peer_base, std::uintptr_t src, bool ping, size_t bytes, int warmup,
         int reps, int workgroups, double timeout_s, std::uintptr_t s) {
        IpcPingPongConfig cfg;
        cfg.bytes = bytes;
        cfg.warmup = warmup;
        cfg.reps = reps;
        cfg.workgroups = workgroups;
        cfg.timeout_s = timeout_s;
        return pingpong_ipc(mine, ptr<unsigned char>(peer_base), ptr<void>(src), ping, cfg, strm(s));
      },
      py::arg("mailbox"), py::arg("peer_base"), py::arg("src"), py::arg("ping"), py::arg("nbytes"),
      py::arg("warmup") = 5, py::arg("reps") = 50, py::arg("workgroups") = 0, py::arg("timeout_s") = 20.0,
      py::arg("stream") = 0, py::call_guard<py::gil_scoped_release>());
  m.def("pingpong_ipc_loopback", &pingpong_ipc_loopback, py::arg("nbytes"), py::arg("warmup") = 5,
        py::arg("reps") = 50, py::arg("workgroups") = 0, py::call_guard<py::gil_scoped_release>());
  // Copy-engine ping-pong (SDMA copies into the peer's IPC-mapped mailbox).
  m.def(
      "pingpong_peer_copy",
      [](const IpcMailbox& mine, std::uintptr_t peer_base, std::uintptr_t src, bool ping, size_t bytes, int warmup,
         int reps, PingPongMode mode, double timeout_s, std::uintptr_t s) {
        PeerCopyConfig cfg;
        cfg.bytes = bytes;
        cfg.warmup = warmup;
        cfg.reps = reps;
        cfg.mode = mode;
        cfg.timeout_s = timeout_s;
        return pingpong_peer_copy(mine, ptr<unsigned char>(peer_base), ptr<void>(src), ping, cfg, strm(s));
      },
      py::arg("mailbox"), py::arg("peer_base"), py::arg("src"), py::arg("ping"), py::arg("nbytes"),
      py::arg("warmup") = 3, py::arg("reps") = 20, py::arg("mode") = PingPongMode::Async, py::arg("timeout_s") = 20.0,
      py::arg("stream") = 0, py::call_guard<py::gil_scoped_release>());
  m.def("pingpong_peer_copy_local", &pingpong_peer_copy_local, py::arg("nbytes"), py::arg("warmup") = 3,
        py::arg("reps") = 20, py::arg("dev_a") = 0, py::arg("dev_b") = 0, py::call_guard<py::gil_scoped_release>(),
        "one process: the copy-engine protocol between two local mailboxes (dev_a != dev_b: hipMemcpyPeerAsync)");
}
