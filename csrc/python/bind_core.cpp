// _mxs_core: host-only bindings of the layout / region / topology / halo-plan
// library (no HIP, no MPI), so CPU-only tests and the gloo halo backend share
// exactly the plan the GPU and MPI backends execute.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <array>
#include <sstream>

#include "mxs/core/error.hpp"
#include "mxs/grid/layout.hpp"
#include "mxs/grid/regions.hpp"
#include "mxs/halo/plan.hpp"
#include "mxs/kernels/cg.hpp"
#include "mxs/kernels/chunk_schedule.hpp"
#include "mxs/kernels/fixed_edge_split.hpp"
#include "mxs/kernels/heat.hpp"
#include "mxs/kernels/multigrid.hpp"
#include "mxs/kernels/pcg.hpp"
#include "mxs/kernels/relaxation.hpp"
#include "mxs/runtime/call_plan.hpp"
#include "mxs/runtime/decision.hpp"
#include "mxs/topo/cart.hpp"

namespace py = pybind11;
using namespace mxs;

PYBIND11_MODULE(_mxs_core, m) {
  m.doc() = "mxs host-side core: layouts, regions, Cartesian topology, halo plans";

  py::class_<Array2D>(m, "Array2D")
      .def(py::init<index_t, index_t, index_t, index_t, index_t>(), py::arg("width"), py::arg("height"),
           py::arg("row_stride"), py::arg("x_offset") = 0, py::arg("y_offset") = 0)
      .def_readwrite("width", &Array2D::width)
      .def_readwrite("height", &Array2D::height)
      .def_readwrite("x_offset", &Array2D::x_offset)
      .def_readwrite("y_offset", &Array2D::y_offset)
      .def_readwrite("row_stride", &Array2D::row_stride)
      .def("size", &Array2D::size)
      .def("index", &Array2D::index)
      .def("__eq__", [](const Array2D& a, const Array2D& b) { return a == b; })
      .def("__str__", [](const Array2D& a) {
        std::ostringstream os;
        os << a;
        return os.str();
      })
      .def("__repr__", [](const Array2D& a) {
        std::ostringstream os;
        os << "Array2D(" << a << ", stride: " << a.row_stride << ")";
        return os.str();
      });

  py::class_<TileGeom>(m, "TileGeom")
      .def(py::init<>())
      .def_readwrite("width", &TileGeom::width)
      .def_readwrite("height", &TileGeom::height)
      .def_readwrite("halo_x", &TileGeom::halo_x)
      .def_readwrite("halo_y", &TileGeom::halo_y)
      .def_readwrite("pitch", &TileGeom::pitch)
      .def_readwrite("x_origin", &TileGeom::x_origin)
      .def("total_width", &TileGeom::total_width)
      .def("total_height", &TileGeom::total_height)
      .def("alloc_elems", &TileGeom::alloc_elems)
      .def("full", &TileGeom::full)
      .def("core", &TileGeom::core)
      .def("core_offset", &TileGeom::core_offset)
      .def_static("compact", &TileGeom::compact, py::arg("width"), py::arg("height"), py::arg("halo_x"),
                  py::arg("halo_y"))
      .def_static("aligned", &TileGeom::aligned, py::arg("width"), py::arg("height"), py::arg("halo_x"),
                  py::arg("halo_y"), py::arg("elem_bytes"), py::arg("align_bytes") = 16,
                  py::arg("pitch_align_bytes") = 256)
      .def("__eq__", [](const TileGeom& a, const TileGeom& b) { return a == b; })
      .def("__repr__", [](const TileGeom& g) {
        std::ostringstream os;
        os << "TileGeom(width=" << g.width << ", height=" << g.height << ", halo=(" << g.halo_x << ", "
           << g.halo_y << "), pitch=" << g.pitch << ", x_origin=" << g.x_origin << ")";
        return os.str();
      });

  py::enum_<RegionID>(m, "RegionID")
      .value("TOP_LEFT", TOP_LEFT)
      .value("TOP_CENTER", TOP_CENTER)
      .value("TOP_RIGHT", TOP_RIGHT)
      .value("CENTER_LEFT", CENTER_LEFT)
      .value("CENTER", CENTER)
      .value("CENTER_RIGHT", CENTER_RIGHT)
      .value("BOTTOM_LEFT", BOTTOM_LEFT)
      .value("BOTTOM_CENTER", BOTTOM_CENTER)
      .value("BOTTOM_RIGHT", BOTTOM_RIGHT)
      .value("TOP", TOP)
      .value("LEFT", LEFT)
      .value("BOTTOM", BOTTOM)
      .value("RIGHT", RIGHT);
  m.def("region_name", [](RegionID r) { return std::string(region_name(r)); });
  m.def("sub_array_region", &sub_array_region, py::arg("grid"), py::arg("stencil_width"),
        py::arg("stencil_height"), py::arg("region"));
  m.def("send_region", &send_region);
  m.def("recv_region", &recv_region);
  m.attr("NUM_DIRS") = kNumDirs;
  m.def("dir_offset", [](int d) {
    auto o = dir_offset(d);
    return py::make_tuple(o.dx, o.dy);
  });
  m.def("dir_opposite", &dir_opposite);
  m.def("dir_name", [](int d) { return std::string(dir_name(d)); });
  m.def("dir_is_corner", &dir_is_corner);
  m.def("reference_tag", &reference_tag);

  m.attr("PROC_NULL") = kProcNull;
  py::class_<CartTopology>(m, "CartTopology")
      .def(py::init<int, int, bool, bool>(), py::arg("rows"), py::arg("cols"), py::arg("periodic_rows") = true,
           py::arg("periodic_cols") = true)
      .def_readonly("rows", &CartTopology::rows)
      .def_readonly("cols", &CartTopology::cols)
      .def_readonly("periodic_rows", &CartTopology::periodic_rows)
      .def_readonly("periodic_cols", &CartTopology::periodic_cols)
      .def("size", &CartTopology::size)
      .def("coords", [](const CartTopology& t, int r) {
        auto c = t.coords(r);
        return py::make_tuple(c[0], c[1]);
      })
      .def("rank_of", &CartTopology::rank_of)
      .def("shift", &CartTopology::shift, py::arg("rank"), py::arg("dx"), py::arg("dy"))
      .def("neighbor", &CartTopology::neighbor)
      .def("cart_shift", [](const CartTopology& t, int rank, int dim, int disp) {
        auto s = t.cart_shift(rank, dim, disp);
        return py::make_tuple(s[0], s[1]);
      })
      .def("grid_text", [](const CartTopology& t) {
        std::ostringstream os;
        print_cartesian_grid(os, t);
        return os.str();
      });
  m.def("dims_create", [](int n) {
    auto d = dims_create(n);
    return py::make_tuple(d[0], d[1]);
  });
  m.def("block_split", [](index_t n, int p, int i) {
    auto b = block_split(n, p, i);
    return py::make_tuple(b.start, b.len);
  });

  py::class_<HaloSegment>(m, "HaloSegment")
      .def_readonly("dir", &HaloSegment::dir)
      .def_readonly("region", &HaloSegment::region)
      .def_readonly("offset", &HaloSegment::offset);
  py::class_<HaloMessage>(m, "HaloMessage")
      .def_readonly("peer", &HaloMessage::peer)
      .def_readonly("offset", &HaloMessage::offset)
      .def_readonly("count", &HaloMessage::count)
      .def_readonly("segments", &HaloMessage::segments);
  py::class_<HaloCopy>(m, "HaloCopy")
      .def_readonly("dir", &HaloCopy::dir)
      .def_readonly("src", &HaloCopy::src)
      .def_readonly("dst", &HaloCopy::dst);
  py::class_<HaloPlan>(m, "HaloPlan")
      .def_readonly("tile", &HaloPlan::tile)
      .def_readonly("rank", &HaloPlan::rank)
      .def_readonly("corners", &HaloPlan::corners)
      .def_readonly("sends", &HaloPlan::sends)
      .def_readonly("recvs", &HaloPlan::recvs)
      .def_readonly("self_copies", &HaloPlan::self_copies)
      .def_readonly("send_elems", &HaloPlan::send_elems)
      .def_readonly("recv_elems", &HaloPlan::recv_elems);
  m.def("make_halo_plan", &make_halo_plan, py::arg("topo"), py::arg("rank"), py::arg("tile"),
        py::arg("corners") = true, py::arg("loopback_self") = false);
  m.def(
      "paired_decision",
      [](std::vector<double> ratios, double min_gain) {
        const int n = int(ratios.size());
        const auto [med, iqr] = median_iqr(ratios);
        py::dict d;
        d["median"] = med;
        d["iqr"] = iqr;
        d["notch"] = median_notch(med, iqr, n);
        d["win"] = paired_win(med, iqr, n, min_gain);
        return d;
      },
      py::arg("ratios"), py::arg("min_gain") = 0.0,
      "the solver's opening / direct-halo rule on per-round ratios candidate / baseline (runtime/decision.hpp)");
  m.def(
      "opening_rule",
      [](double lead_frac) { return opening_rule(lead_frac) == WinRule::Median ? "median" : "notch"; },
      py::arg("lead_frac"),
      "the opening decision's rule for a measured exchange lead / pass: median (a tie goes to interior-first) "
      "or notch");
  m.def(
      "opening_decision",
      [](const std::vector<std::vector<double>>& serial, const std::vector<std::vector<std::vector<double>>>& cands,
         double min_gain, const std::string& rule) {
        // serial[rank][round], cands[rank][candidate][round]: what every rank timed.
        // The solver agrees the element-wise max (one vector per rank), then decides.
        MXS_CHECK(!serial.empty() && serial.size() == cands.size(), "one serial and one candidate set per rank");
        const size_t nr = serial[0].size(), nc = cands[0].size();
        std::vector<std::vector<double>> flat(serial.size());
        for (size_t r = 0; r < serial.size(); ++r) {
          MXS_CHECK(serial[r].size() == nr && cands[r].size() == nc, "ranks must time the same rounds and slots");
          flat[r] = serial[r];
          for (const auto& c : cands[r]) {
            MXS_CHECK(c.size() == nr, "ranks must time the same rounds");
            flat[r].insert(flat[r].end(), c.begin(), c.end());
          }
        }
        const std::vector<double> v = elementwise_max(flat);
        std::vector<std::vector<double>> cm(nc);
        for (size_t c = 0; c < nc; ++c) cm[c].assign(v.begin() + (1 + c) * nr, v.begin() + (2 + c) * nr);
        MXS_CHECK(rule == "median" || rule == "notch", "rule: median (the opening) or notch");
        const RoundDecision d = decide_on_maxima(std::vector<double>(v.begin(), v.begin() + nr), cm, min_gain,
                                                 rule == "median" ? WinRule::Median : WinRule::Notch);
        py::dict out;
        out["best"] = d.best;
        out["win"] = d.win;
        out["ratio"] = d.ratio;
        out["ratio_iqr"] = d.ratio_iqr;
        out["notch"] = d.notch;
        out["serial_ms"] = d.baseline_ms;
        out["candidate_ms"] = d.candidate_ms;
        out["ratios"] = d.ratios;
        return out;
      },
      py::arg("serial"), py::arg("candidates"), py::arg("min_gain") = 0.0, py::arg("rule") = "median",
      "StencilSolver::choose_opening's collective rule: per-round maxima over ranks, paired ratios of the maxima, "
      "the lowest notch among candidates, which wins when its median ratio is <= 1 - min_gain (rule 'median', the "
      "opening) or its notch is below it (rule 'notch', the steady and direct-halo decisions) "
      "(runtime/decision.hpp); missing slots: kMissingSample");
  m.def(
      "plan_call",
      [](int iters, int block, const std::string& mode, bool multi_rank, bool opening_on, bool steady_on,
         bool ghost_fresh) {
        MXS_CHECK(block >= 1, "plan_call: block must be >= 1");
        const SuperstepMode md = mode == "fused"           ? SuperstepMode::Fused
                                 : mode == "direct"        ? SuperstepMode::Direct
                                 : mode == "overlap"       ? SuperstepMode::Overlap
                                 : mode == "post-exchange" ? SuperstepMode::PostExchange
                                                           : throw std::invalid_argument(
                                                                 "mode must be fused, direct, overlap or post-exchange");
        const CallPlan p = plan_call(iters, block, md, multi_rank, opening_on, steady_on, ghost_fresh);
        static const char* const kinds[] = {"opening", "prime", "full", "bare"};
        py::list steps, blocks;
        for (int i = 0; i < p.n_steps; ++i)
          steps.append(py::make_tuple(kinds[int(p.steps[i].kind)], p.steps[i].S, p.steps[i].count));
        for (int i = 0; i < p.n_blocks; ++i) blocks.append(py::make_tuple(p.blocks[i].S, p.blocks[i].count));
        py::dict d;
        d["steps"] = steps;
        d["blocks"] = blocks;
        d["exchanges"] = p.exchanges;
        // "primed": "interior-first" where the rank has the form at the first step's depth, else "serial".
        d["label"] = p.label == OpeningLabel::Primed ? "primed" : to_string(p.label, false);
        return d;
      },
      py::arg("iters"), py::arg("block"), py::arg("mode") = "post-exchange", py::arg("multi_rank") = false,
      py::arg("opening_on") = false, py::arg("steady_on") = false, py::arg("ghost_fresh") = false,
      "the steps of StencilSolver::run(iters) (runtime/call_plan.hpp): (kind, S, count) with kind opening | prime | "
      "full | bare, the (S, count) blocks, the halo exchanges the call issues and its opening's label");
  m.attr("MISSING_SAMPLE") = kMissingSample;
  m.attr("HOLD_TOP") = unsigned(kernels::kHoldTop);
  m.attr("HOLD_BOTTOM") = unsigned(kernels::kHoldBottom);
  m.attr("HOLD_LEFT") = unsigned(kernels::kHoldLeft);
  m.attr("HOLD_RIGHT") = unsigned(kernels::kHoldRight);
  m.def(
      "fixed_edge_split",
      [](index_t w, index_t h, int S, int vec, unsigned hold) {
        const kernels::FixedEdgeSplit sp = kernels::fixed_edge_split(w, h, S, vec, hold);
        auto rect = [](const kernels::Rect& r) { return py::make_tuple(r.x0, r.x1, r.y0, r.y1); };
        py::list frame;
        for (int i = 0; i < sp.n_frame; ++i) frame.append(rect(sp.frame[i]));
        py::dict d;
        d["interior"] = rect(sp.interior);
        d["frame"] = frame;
        return d;
      },
      py::arg("width"), py::arg("height"), py::arg("steps"), py::arg("vec"), py::arg("hold"),
      "time blocking beside fixed edges: the core's interior (x0, x1, y0, y1), shrunk by `steps` on the held sides "
      "(HOLD_* bits; left / right to whole `vec`-cell vectors), and the frame rectangles that cover the rest "
      "(kernels/fixed_edge_split.hpp); an empty interior is (0, 0, 0, 0)");
  m.def(
      "chebyshev_cycle",
      [](long long w, long long h, double c0, double c1, int M) {
        const kernels::LevelTable t = kernels::chebyshev_cycle(w, h, c0, c1, M);
        py::dict d;
        d["n"] = t.n;
        d["center"] = std::vector<double>(t.center, t.center + t.n);
        d["neighbor"] = std::vector<double>(t.neighbor, t.neighbor + t.n);
        d["growth"] = t.growth;
        return d;
      },
      py::arg("global_width"), py::arg("global_height"), py::arg("c_center"), py::arg("c_neighbor"), py::arg("levels"),
      "the Chebyshev relaxation cycle of `levels` levels for a grid with fixed edges (kernels/relaxation.hpp): "
      "per-level (center, neighbor) coefficients in Leja order and the prefix-polynomial growth; raises ValueError "
      "unless c_neighbor != 0 and the spectrum of I - A is positive");
  m.attr("MAX_LEVELS") = kernels::kMaxLevels;
  // Multigrid: the level planner and the sweep tables (kernels/multigrid.hpp).
  m.def(
      "mg_plan_levels",
      [](long long w, long long h) {
        std::vector<std::pair<long long, long long>> out;
        for (const kernels::MgLevel& l : kernels::mg_plan_levels(w, h)) out.emplace_back(l.width, l.height);
        return out;
      },
      py::arg("width"), py::arg("height"),
      "the multigrid levels of a width x height core, finest first, as (width, height) pairs: vertex-centred "
      "coarsening (n - 1) / 2 of both axes together while both sides are odd, >= 3 and the larger is above 31; "
      "raises ValueError when the coarsest level is above 63 on a side (the message names the nearest sizes that work)");
  m.def("mg_check_operator", &kernels::mg_check_operator, py::arg("c_center"), py::arg("c_neighbor"),
        "raises ValueError unless |c_center + 4 c_neighbor - 1| <= 1e-12 and c_neighbor > 0");
  auto sweep_dict = [](const kernels::MgSweepTable& t) {
    py::dict d;
    d["n"] = t.n;
    d["center"] = std::vector<double>(t.center, t.center + t.n);
    d["neighbor"] = std::vector<double>(t.neighbor, t.neighbor + t.n);
    d["weight"] = std::vector<double>(t.weight, t.weight + t.n);
    return d;
  };
  m.def(
      "mg_smoother_table",
      [sweep_dict](double c0, double c1, double omega, int sweeps) {
        return sweep_dict(kernels::mg_smoother_table(c0, c1, omega, sweeps));
      },
      py::arg("c_center"), py::arg("c_neighbor"), py::arg("omega"), py::arg("sweeps"),
      "the damped-Jacobi smoother's per-sweep (center, neighbor, weight) table");
  m.def(
      "mg_coarse_plan",
      [sweep_dict](long long w, long long h, double c0, double c1, double reduction) {
        const kernels::MgCoarsePlan p = kernels::mg_coarse_plan(w, h, c0, c1, reduction);
        py::dict d = sweep_dict(p.table);
        d["repeats"] = p.repeats;
        d["rho"] = p.rho;
        return d;
      },
      py::arg("width"), py::arg("height"), py::arg("c_center"), py::arg("c_neighbor"), py::arg("coarse_reduction"),
      "the coarsest level's solve: the 32-level Leja-ordered Chebyshev cycle as a sweep table, its error bound rho "
      "and the smallest repeat count with rho^repeats <= coarse_reduction");
  // Conjugate gradients (kernels/cg.hpp).
  m.def(
      "cg_check_sides",
      [](double c0, double c1, const std::vector<std::string>& neumann) {
        kernels::cg_check_sides(c0, c1, kernels::ghost_sides_of(neumann));
      },
      py::arg("c_center"), py::arg("c_neighbor"), py::arg("neumann") = std::vector<std::string>{},
      "cg_check_operator, plus: unknown or repeated side names raise, and so do four Neumann sides with "
      "c_center + 4 c_neighbor = 1 (the operator is then singular)");
  m.def("cg_check_operator", &kernels::cg_check_operator, py::arg("c_center"), py::arg("c_neighbor"),
        "raises ValueError unless c_neighbor > 0 and c_center + 4 c_neighbor <= 1 + 1e-12 (then (1 - c_center) v - "
        "c_neighbor (n + s + w + e) is symmetric positive definite)");
  // Implicit heat steps (kernels/heat.hpp).
  m.def(
      "heat_coefficients",
      [](double lam, double theta) {
        const kernels::HeatCoeffs h = kernels::heat_coefficients(lam, theta);
        py::dict d;
        d["c1"] = h.c1;
        d["a"] = h.a;
        d["b"] = h.b;
        d["s"] = h.s;
        return d;
      },
      py::arg("lam"), py::arg("theta") = 1.0,
      "the theta-scheme step as the fixed-edge problem u' = A u' + g: {c1, a, b, s} with D = 1 + 4 theta lam, c1 = theta "
      "lam / D (c_center = 0), g = a u + b (n + s + w + e) + s q, s = 1 / D; raises ValueError for lam <= 0, non-finite "
      "input or theta outside [0.5, 1]");
  // Preconditioned CG (kernels/pcg.hpp): the any-size level plan and the coarse solve plan.
  auto pcg_level_dict = [](const kernels::PcgLevel& l) {
    py::dict d;
    d["width"] = l.width;
    d["height"] = l.height;
    d["reflect_rows"] = l.reflect_rows;
    d["reflect_cols"] = l.reflect_cols;
    d["c_center"] = l.c0;
    d["top"] = l.sides.top;
    d["bottom"] = l.sides.bottom;
    d["left"] = l.sides.left;
    d["right"] = l.sides.right;
    return d;
  };
  m.def(
      "pcg_plan_levels",
      [pcg_level_dict](long long w, long long h, double c0, double c1, const std::vector<std::string>& neumann) {
        py::list out;
        for (const kernels::PcgLevel& l : kernels::pcg_plan_levels(w, h, c0, c1, kernels::ghost_sides_of(neumann)))
          out.append(pcg_level_dict(l));
        return out;
      },
      py::arg("width"), py::arg("height"), py::arg("c_center") = 0.2, py::arg("c_neighbor") = 0.2,
      py::arg("neumann") = std::vector<std::string>{},
      "the preconditioner's levels of a width x height core, finest first, as dicts (width, height, reflect_rows, "
      "reflect_cols, c_center): n_c = floor(n / 2) on both axes while the larger side is above 31 and the smaller at "
      "least 2; a flag is set when the parent's height (rows) or width (cols) was even; raises ValueError when the "
      "coarsest level is above 63 on a side (the message names ConjugateGradient2D)");
  // `sides`: the four ghost codes (top, bottom, left, right); a set flag makes a far code of 0 a -1.
  auto pcg_level_of = [](long long w, long long h, bool rr, bool rc, double c0, const std::array<int, 4>& sides) {
    return kernels::pcg_level_of(w, h, rr, rc, c0, kernels::GhostSides{sides[0], sides[1], sides[2], sides[3]});
  };
  const std::array<int, 4> no_sides{0, 0, 0, 0};
  m.def(
      "pcg_coarse_interval",
      [pcg_level_of](long long w, long long h, bool rr, bool rc, double c0, double c1, const std::array<int, 4>& sides) {
        const kernels::RelaxSpectrum sp = kernels::pcg_coarse_interval(pcg_level_of(w, h, rr, rc, c0, sides), c1);
        return std::make_pair(sp.a, sp.b);
      },
      py::arg("width"), py::arg("height"), py::arg("reflect_rows"), py::arg("reflect_cols"), py::arg("c_center"),
      py::arg("c_neighbor"), py::arg("sides") = no_sides,
      "(a, b) the coarse solve of a level is built on: relaxation_spectrum's, with the Gershgorin upper end "
      "1 - c_center + 4 c_neighbor when a side reflects");
  m.def(
      "pcg_coarse_plan",
      [sweep_dict, pcg_level_of](long long w, long long h, bool rr, bool rc, double c0, double c1, double reduction,
                                 const std::array<int, 4>& sides) {
        const kernels::MgCoarsePlan p = kernels::pcg_coarse_plan(pcg_level_of(w, h, rr, rc, c0, sides), c1, reduction);
        py::dict d = sweep_dict(p.table);
        d["repeats"] = p.repeats;
        d["rho"] = p.rho;
        return d;
      },
      py::arg("width"), py::arg("height"), py::arg("reflect_rows"), py::arg("reflect_cols"), py::arg("c_center"),
      py::arg("c_neighbor"), py::arg("coarse_reduction"), py::arg("sides") = no_sides,
      "the coarsest level's solve: mg_coarse_plan without a reflecting or mirror side, else the 32-level cycle of pcg_coarse_interval");
  m.def(
      "chebyshev_cycle_interval",
      [](double a, double b, double c0, double c1, int M) {
        const kernels::LevelTable t = kernels::chebyshev_cycle_interval(a, b, c0, c1, M);
        py::dict d;
        d["n"] = t.n;
        d["center"] = std::vector<double>(t.center, t.center + t.n);
        d["neighbor"] = std::vector<double>(t.neighbor, t.neighbor + t.n);
        d["growth"] = t.growth;
        return d;
      },
      py::arg("a"), py::arg("b"), py::arg("c_center"), py::arg("c_neighbor"), py::arg("levels"),
      "chebyshev_cycle on a given interval 0 < a < b of I - A: the same roots, Leja order and tables");
  m.attr("PCG_SCALARS_BYTES") = int(sizeof(kernels::PcgScalars));
  m.attr("MG_COARSEN_ABOVE") = kernels::kMgCoarsenAbove;
  m.attr("MG_COARSEST_MAX") = kernels::kMgCoarsestMax;
  m.attr("MG_MAX_SMOOTH") = kernels::kMgMaxSmooth;
  m.def("balanced_starts", &kernels::balanced_starts, py::arg("groups"), py::arg("rows"), py::arg("blocks"),
        py::arg("fill"), py::arg("last_rows") = 0,
        "fill-aware linear starts of the pipeline workgroups' shares (blocks + 1 entries); last_rows > 0: the last "
        "group's run is that long (the split narrow group), 0 = rows");
  // Interior-first (halo-last) schedule of the multi-GPU opening super-step.
  m.def(
      "halo_last_schedule",
      [](std::int64_t groups, std::int64_t rows, int blocks, std::int64_t fill, std::int64_t depth,
         std::vector<std::uint8_t> ghost, int outer_wgs, double lead_frac, std::int64_t band_rows, int granule, int min_outer) {
        const auto h = kernels::make_halo_last_schedule(groups, rows, blocks, fill, depth, ghost, outer_wgs, lead_frac,
                                                        band_rows, granule, min_outer);
        auto lists = [](const kernels::ChunkSchedule& s) {
          py::list table;
          for (int w = 0; w < s.blocks; ++w) {
            py::list l;
            for (int e = 0; e < s.entries; ++e) {
              const auto& c = s.at(w, e);
              if (c.r1 > c.r0) l.append(py::make_tuple(c.group, c.r0, c.r1));
            }
            table.append(l);
          }
          return table;
        };
        py::dict d;
        d["inner"] = lists(h.inner);
        d["outer"] = lists(h.outer);
        d["hf"] = h.hf;
        d["inner_cost"] = h.inner_cost;
        d["outer_cost"] = h.outer_cost;
        d["serial_cost"] = h.serial_cost;
        d["moved_rows"] = h.moved_rows;
        d["band"] = h.band;
        d["check"] = kernels::check_halo_last_schedule(h, groups, rows, depth, ghost);
        return d;
      },
      py::arg("groups"), py::arg("rows"), py::arg("blocks"), py::arg("fill"), py::arg("depth"), py::arg("ghost"),
      py::arg("outer_wgs") = 0, py::arg("lead_frac") = 0.12, py::arg("band_rows") = 0, py::arg("granule") = 1,
      py::arg("min_outer") = 1,
      "inner / outer chunk lists (group, r0, r1) of the interior-first pass + the check ('' = ok)");
}
