// Host-only unit tests of the C++ core ("Unit tests"): region
// algebra, accessor indexing, Cartesian neighbour tables, halo-plan
// aggregation/ordering, the collective decision statistics, the
// interior-first chunk schedule, the pipeline form rule, the fast-form guard,
// the solver's call plan and the CG solvers' host protocol. Run by ctest and by
// tests/test_cpp_unit.py (and under host ASan/UBSan by scripts/cpu_sanitize.sh).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>
#include <vector>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>

#include "mxs/grid/layout.hpp"
#include "mxs/grid/print.hpp"
#include "mxs/grid/regions.hpp"
#include "mxs/halo/plan.hpp"
#include "mxs/kernels/chunk_schedule.hpp"
#include "mxs/kernels/kernels.hpp"
#include "mxs/kernels/pipe_form.hpp"
#include "mxs/runtime/call_plan.hpp"
#include "mxs/runtime/cg_protocol.hpp"
#include "mxs/runtime/decision.hpp"
#include "mxs/topo/cart.hpp"

using namespace mxs;

static int g_failures = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: EXPECT failed: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failures;                                                     \
    }                                                                   \
  } while (0)

static std::string str(const Array2D& a) {
  std::ostringstream os;
  os << a;
  return os.str();
}

static void test_regions() {
  // 20x20 tile of the reference default (16x16 core, 5x5 stencil).
  const Array2D g(20, 20, 20);
  EXPECT(str(sub_array_region(g, 5, 5, CENTER)) == "width:  16, height: 16, x offset: 2, y offset: 2");
  EXPECT(str(sub_array_region(g, 5, 5, TOP_LEFT)) == "width:  2, height: 2, x offset: 0, y offset: 0");
  EXPECT(str(sub_array_region(g, 5, 5, BOTTOM_CENTER)) == "width:  16, height: 2, x offset: 2, y offset: 18");
  EXPECT(str(sub_array_region(g, 5, 5, RIGHT)) == "width:  2, height: 20, x offset: 18, y offset: 0");
  // TestSubRegionExtraction values quoted in SURVEY §4.
  std::ostringstream os;
  test_subregion_extraction(os);
  const std::string t = os.str();
  EXPECT(t.find("Width: 34, Height: 34") != std::string::npos);
  EXPECT(t.find("top center:    width:  30, height: 2, x offset: 2, y offset: 0") != std::string::npos);
  EXPECT(t.find("top:           width:  30, height: 2, x offset: 2, y offset: 2") != std::string::npos);
}

static void test_layout() {
  const TileGeom g = TileGeom::aligned(8192, 8192, 1, 1, 4);
  EXPECT((g.x_origin + g.halo_x) % 4 == 0);
  EXPECT(g.pitch % 64 == 0);
  EXPECT(g.pitch >= g.x_origin + g.halo_x + 8192 + 4);
  const TileGeom c = TileGeom::compact(16, 16, 2, 2);
  EXPECT(c.pitch == 20 && c.core_offset() == 2 * 20 + 2);
  double buf[400];
  for (int i = 0; i < 400; ++i) buf[i] = i;
  Accessor2D<double> a(buf, c.core());
  EXPECT(a(0, 0) == 42 && a(3, 1) == 42 + 20 + 3);
  // send/recv regions of an aligned tile
  const Array2D top_send = send_region(g, D_TOP);
  EXPECT(top_send.width == 8192 && top_send.height == 1 && top_send.y_offset == 1);
  const Array2D left_recv = recv_region(g, D_LEFT);
  EXPECT(left_recv.width == 1 && left_recv.x_offset == g.x_origin && left_recv.y_offset == 1);
}

static void test_cart() {
  auto d = dims_create(8);
  EXPECT(d[0] == 4 && d[1] == 2);
  d = dims_create(9);
  EXPECT(d[0] == 3 && d[1] == 3);
  d = dims_create(7);
  EXPECT(d[0] == 7 && d[1] == 1);
  const CartTopology t(3, 3);
  // rank 4 = centre of a 3x3 periodic grid; its 8 neighbours are all others.
  std::set<int> n;
  for (int dd = 0; dd < kNumDirs; ++dd) n.insert(t.neighbor(4, dd));
  EXPECT(n.size() == 8 && !n.count(4));
  EXPECT(t.neighbor(0, D_TOP_LEFT) == 8);  // periodic wrap
  const CartTopology np(3, 3, false, false);
  EXPECT(np.neighbor(0, D_TOP) == kProcNull);
  auto s = np.cart_shift(4, 0, 1);
  EXPECT(s[0] == 1 && s[1] == 7);  // mpi10.cpp: rank 4 neighbours 1,7,3,5
  s = np.cart_shift(4, 1, 1);
  EXPECT(s[0] == 3 && s[1] == 5);
  std::ostringstream os;
  print_cartesian_grid(os, t);
  EXPECT(os.str() == "0 1 2 \n3 4 5 \n6 7 8 \n");
  auto b = block_split(10, 3, 0);
  EXPECT(b.start == 0 && b.len == 4);
  b = block_split(10, 3, 2);
  EXPECT(b.start == 7 && b.len == 3);
}

static void test_plan() {
  const TileGeom g = TileGeom::compact(16, 16, 2, 2);
  // 3x3: 8 distinct peers, one segment each, no self copies.
  HaloPlan p = make_halo_plan(CartTopology(3, 3), 4, g);
  EXPECT(p.sends.size() == 8 && p.self_copies.empty());
  for (const auto& m : p.sends) EXPECT(m.segments.size() == 1);
  EXPECT(p.send_elems == 4 * 4 + 4 * 32 && p.recv_elems == p.send_elems);
  // 1x1: everything is a self copy.
  p = make_halo_plan(CartTopology(1, 1), 0, g);
  EXPECT(p.sends.empty() && p.self_copies.size() == 8);
  // 2x4 periodic (the 8-GPU config): 5 distinct peers; up == down.
  const CartTopology t24(2, 4);
  p = make_halo_plan(t24, 1, g);
  EXPECT(p.sends.size() == 5);
  for (const auto& m : p.sends) {
    // Symmetry: what I send to m.peer equals, segment by segment, what m.peer
    // expects from me.
    const HaloPlan q = make_halo_plan(t24, m.peer, g);
    bool found = false;
    for (const auto& r : q.recvs) {
      if (r.peer != 1) continue;
      found = true;
      EXPECT(r.count == m.count && r.segments.size() == m.segments.size());
      for (size_t i = 0; i < r.segments.size() && i < m.segments.size(); ++i) {
        EXPECT(r.segments[i].dir == m.segments[i].dir);
        EXPECT(r.segments[i].region.size() == m.segments[i].region.size());
      }
    }
    EXPECT(found);
  }
  // Star (no corners): 4 directions.
  p = make_halo_plan(CartTopology(3, 3), 4, g, /*corners=*/false);
  EXPECT(p.sends.size() == 4);
  // Loopback routes self through the wire.
  p = make_halo_plan(CartTopology(1, 1), 0, g, true, /*loopback_self=*/true);
  EXPECT(p.sends.size() == 1 && p.sends[0].peer == 0 && p.sends[0].segments.size() == 8 && p.self_copies.empty());
  EXPECT(reference_tag(D_TOP) == TOP && reference_tag(D_BOTTOM_RIGHT) == BOTTOM_RIGHT);
}

static void test_decision() {
  // 20 rounds; the baseline drifts between rounds, the candidate stays 5% faster in each.
  std::vector<double> base, fast, slow, missing;
  for (int r = 0; r < 20; ++r) {
    const double clock = 1.0 + 0.1 * ((r * 7) % 5);
    base.push_back(0.30 * clock);
    fast.push_back(0.285 * clock);
    slow.push_back(0.33 * clock);
    missing.push_back(r == 3 ? kMissingSample : 0.2 * clock);
  }
  RoundDecision d = decide_on_maxima(base, {slow, fast, missing}, 0.0);
  EXPECT(d.best == 1 && d.win && std::fabs(d.ratio - 0.95) < 1e-9 && d.ratio_iqr < 1e-9);
  EXPECT(d.ratios[2].empty() && d.ratios[0].size() == 20);  // a missing sample drops the candidate
  EXPECT(!decide_on_maxima(base, {slow}, 0.0).win);
  EXPECT(!decide_on_maxima(base, {fast}, 0.06).win);  // a 5% gain does not meet a 6% margin
  // Element-wise max over ranks: one rank in a fast-serial state does not veto.
  const std::vector<double> r0{0.30, 0.30}, r1{0.25, 0.28};
  const std::vector<double> m = elementwise_max({r0, r1});
  EXPECT(m.size() == 2 && m[0] == 0.30 && m[1] == 0.30);
  std::vector<double> v{3, 1, 2, 4};
  const auto mi = median_iqr(v);
  EXPECT(mi.first == 3 && mi.second == 4 - 2);
  EXPECT(std::fabs(median_notch(1.0, 0.1, 25) - 1.0316) < 1e-9);
}

static void test_halo_last_schedule() {
  // 8 column groups x 600 rows, the edge groups reading the ghost columns, 256
  // workgroups, depth 20: both sets cover every row once, inner chunks stay in the core.
  const std::vector<std::uint8_t> ghost{1, 0, 0, 0, 0, 0, 0, 1};
  const auto h = kernels::make_halo_last_schedule(8, 600, 256, 60, 20, ghost, 0, 0.12, 0, 8, 32);
  EXPECT(kernels::check_halo_last_schedule(h, 8, 600, 20, ghost).empty());
  EXPECT(h.outer.blocks % 8 == 0 && h.outer.blocks >= 32 && h.inner.blocks + h.outer.blocks == 256);
  EXPECT(h.band >= 20);
  // A fixed outer set.
  const auto f = kernels::make_halo_last_schedule(8, 600, 256, 60, 20, ghost, 48);
  EXPECT(f.outer.blocks == 48 && kernels::check_halo_last_schedule(f, 8, 600, 20, ghost).empty());
  // Balanced starts: monotone, cover the whole range.
  const auto st = kernels::balanced_starts(9, 8192, 256, 47);
  EXPECT(st.size() == 257 && st.front() == 0 && st.back() == 9 * 8192);
  bool mono = true;
  for (size_t i = 1; i < st.size(); ++i) mono = mono && st[i] >= st[i - 1];
  EXPECT(mono);
}

// The pipeline form rule (kernels/pipe_form.hpp): the forms the measured rule
// picks and the shape numbers that follow, as the kernels' constexpr shapes
// gave them before the rule was stated once.
static void test_pipe_form() {
  using kernels::EvalForm;
  using kernels::PipeForm;
  using kernels::kLagBoth;
  auto pick = [](int eb, int S, EvalForm e, index_t cols = 8192, kernels::PipeSwitches on = {}) {
    return kernels::pipe_form_for(eb, S, e, cols, on);
  };
  auto is = [](const kernels::PipeChoice& c, int s0, int s1, int pf, bool joint, int lag1, EvalForm e) {
    return c.form == PipeForm{s0, s1, pf, joint, lag1} && c.eval == e;
  };
  const kernels::PipeSwitches no_lag{true, false, true}, no_joint{false, true, true};
  for (EvalForm e : {EvalForm::PerStep, EvalForm::Sum, EvalForm::Scaled}) {
    EXPECT(is(pick(4, 20, e, 12284), 8, 12, 6, true, kLagBoth, e));
    EXPECT(is(pick(4, 20, e, 12288), 12, 8, 6, true, kLagBoth, e));
    EXPECT(is(pick(4, 20, e, 8192, no_lag), 12, 8, 6, true, 0, e));
    EXPECT(is(pick(4, 20, e, 32768, no_lag), 12, 8, 6, true, 0, e));
    EXPECT(is(pick(4, 24, e), 12, 12, 6, true, kLagBoth, e));
    EXPECT(is(pick(4, 24, e, 8192, no_lag), 12, 12, 6, true, 0, e));
    EXPECT(is(pick(8, 16, e), 8, 8, 3, true, kLagBoth, e));
    EXPECT(is(pick(8, 16, e, 8192, no_lag), 8, 8, 3, true, 0, e));
  }
  EXPECT(is(pick(4, 20, EvalForm::Sum, 8192, no_joint), 10, 10, 6, false, 0, EvalForm::Sum));
  EXPECT(is(pick(4, 20, EvalForm::PerStep, 8192, no_joint), 11, 9, 6, false, 0, EvalForm::PerStep));
  EXPECT(is(pick(4, 20, EvalForm::Scaled, 8192, no_joint), 11, 9, 6, false, 0, EvalForm::PerStep));
  EXPECT(is(pick(8, 16, EvalForm::Scaled, 8192, no_joint), 8, 8, 3, false, 0, EvalForm::PerStep));
  for (EvalForm e : {EvalForm::PerStep, EvalForm::Sum}) {
    EXPECT(is(pick(4, 28, e), 12, 16, 6, true, 0, e));
    EXPECT(is(pick(4, 32, e), 16, 16, 3, true, 0, e));
    EXPECT(is(pick(8, 12, e), 6, 6, 3, false, 0, e));
    EXPECT(is(pick(8, 9, e), 4, 5, 3, false, 0, e));
  }
  EXPECT(is(pick(4, 28, EvalForm::Scaled), 12, 16, 6, true, 0, EvalForm::PerStep));  // no scaled kernels at 28
  EXPECT(is(pick(4, 17, EvalForm::PerStep), 9, 8, 6, false, 0, EvalForm::PerStep));
  EXPECT(is(pick(4, 17, EvalForm::Sum), 8, 9, 6, false, 0, EvalForm::Sum));
  EXPECT(is(pick(4, 31, EvalForm::PerStep), 16, 15, 3, false, 0, EvalForm::PerStep));
  EXPECT(is(pick(4, 29, EvalForm::PerStep), 15, 14, 3, false, 0, EvalForm::PerStep));
  // Only the fp32 12 + 12 ascending form splits its narrow last group.
  EXPECT(pick(4, 24, EvalForm::Sum).split && !pick(4, 24, EvalForm::Sum, 8192, no_lag).split);
  EXPECT(!pick(4, 24, EvalForm::Sum, 8192, kernels::PipeSwitches{true, true, false}).split);
  EXPECT(!pick(4, 20, EvalForm::Sum, 32768).split && !pick(8, 16, EvalForm::Sum).split);

  // Output columns per group.
  auto owg = [](int s0, int s1) { return kernels::pipe_owg(PipeForm{s0, s1, 6, true, 0}); };
  EXPECT(owg(12, 8) == 912 && owg(12, 12) == 904 && owg(8, 12) == 928);
  EXPECT(owg(12, 16) == 896 && owg(16, 16) == 864 && owg(8, 8) == 944);
  EXPECT(kernels::pipe_owg(PipeForm{10, 10, 6, false, 0}) == 4 * 216);  // per strip: 256 - 2 * 20
  EXPECT(kernels::pipe_owg(PipeForm{9, 8, 6, false, 0}) == 4 * 216);    // S = 17: the apron rounds up to 20
  EXPECT(kernels::pipe_owg(PipeForm{6, 6, 3, false, 0}) == 4 * 232);
  EXPECT(kernels::joint_owg(12, 12, 2) == 440);
  EXPECT(kernels::pipe_groups(PipeForm{12, 12, 6, true, kLagBoth}, 32768) == 37);
  EXPECT(kernels::pipe_groups(PipeForm{12, 8, 6, true, kLagBoth}, 32768) == 36);
  // Read reach: lead A0 + A1, span 3 * OW0 + 256.
  EXPECT(kernels::pipe_apron(PipeForm{12, 8, 6, true, 0}) == 20 && kernels::pipe_read_span(PipeForm{12, 8, 6, true, 0}) == 952);
  EXPECT(kernels::pipe_apron(PipeForm{8, 12, 6, true, 0}) == 20 && kernels::pipe_read_span(PipeForm{8, 12, 6, true, 0}) == 976);
  EXPECT(kernels::pipe_apron(PipeForm{12, 12, 6, true, 0}) == 24 && kernels::pipe_apron(PipeForm{8, 8, 3, true, 0}) == 16);
  EXPECT(kernels::pipe_apron(PipeForm{9, 8, 6, false, 0}) == 20);
  // Fill rows.
  EXPECT(kernels::pipe_fill_rows(PipeForm{12, 8, 6, true, kLagBoth}) == 51);
  EXPECT(kernels::pipe_fill_rows(PipeForm{8, 12, 6, true, kLagBoth}) == 53);
  EXPECT(kernels::pipe_fill_rows(PipeForm{12, 12, 6, true, kLagBoth}) == 59);
  // The split group: 32768 columns leave 224 for the 37th group of 904, 4096 leave 480.
  const auto s24 = pick(4, 24, EvalForm::Sum);
  EXPECT(kernels::pipe_split_half(s24, 32768, 4801) == 2401);
  EXPECT(kernels::pipe_split_half(s24, 36 * 904 + 440, 100) == 50 && kernels::pipe_split_half(s24, 36 * 904 + 441, 100) == 0);
  EXPECT(kernels::pipe_split_half(s24, 4096, 4096) == 0);
  EXPECT(kernels::pipe_split_half(pick(4, 20, EvalForm::Sum, 32768), 32768 - 8, 4096) == 0);
}

// The fast-form guard (kernels.hpp: fast_form_verdict), one verdict per reason.
static void test_fast_form_verdict() {
  using V = kernels::FastFormVerdict;
  using C = kernels::Stencil5Coeffs;
  EXPECT(kernels::fast_form_verdict<float>(C{0.2, 0.2, true, -1.0}, 24) == V::Ok);
  EXPECT(kernels::eval_form<float>(C{0.2, 0.2, true, -1.0}, 24) == kernels::EvalForm::Sum);
  EXPECT(kernels::eval_form<double>(C{0.5, 0.125, true, 1.0}, 16) == kernels::EvalForm::Scaled);
  EXPECT(kernels::fast_form_verdict<float>(C{0.2, 0.2, false, -1.0}, 24) == V::NotFastPair);
  EXPECT(kernels::fast_form_verdict<float>(C{0.5, 0.0, true, -1.0}, 24) == V::NotFastPair);
  EXPECT(kernels::fast_form_verdict<float>(C{0.9, 0.013, true, -1.0}, 20) == V::RangeUnknownGrowth);
  EXPECT(kernels::eval_form<float>(C{0.9, 0.013, true, -1.0}, 20) == kernels::EvalForm::PerStep);
  EXPECT(kernels::fast_form_verdict<float>(C{0.9, 0.013, true, 10.0}, 20) == V::RangeOverflow);  // 73^20 = 2e37
  EXPECT(kernels::fast_form_verdict<float>(C{0.9, 0.013, true, 1.0}, 20) == V::Ok);
  EXPECT(kernels::fast_form_verdict<float>(C{0.3, 0.2, true, 1.0}, 20) == V::Unbounded);
  EXPECT(kernels::fast_form_verdict<float>(C{0.25, 0.25, true, 1.0}, 20) == V::Unbounded);
  EXPECT(kernels::fast_form_verdict<float>(C{0.02, 0.02, true, 1.0}, 24) == V::ScaleSubnormal);  // 0.02^24 = 1.7e-41
  EXPECT(kernels::fast_form_verdict<double>(C{0.02, 0.02, true, 1.0}, 24) == V::Ok);
  for (int S : {16, 20, 24}) {
    const double edge32 = double(std::numeric_limits<float>::max()) / 4.0 / std::pow(5.0, double(S));
    EXPECT(kernels::fast_form_verdict<float>(C{0.2, 0.2, true, edge32 * (1.0 - 1e-9)}, S) == V::Ok);
    EXPECT(kernels::fast_form_verdict<float>(C{0.2, 0.2, true, edge32 * (1.0 + 1e-9)}, S) == V::RangeOverflow);
    const double edge64 = std::numeric_limits<double>::max() / 4.0 / std::pow(5.0, double(S));
    EXPECT(kernels::fast_form_verdict<double>(C{0.2, 0.2, true, edge64 * (1.0 - 1e-9)}, S) == V::Ok);
    EXPECT(kernels::fast_form_verdict<double>(C{0.2, 0.2, true, edge64 * (1.0 + 1e-9)}, S) == V::RangeOverflow);
  }
  EXPECT(kernels::fast_form_verdict<float>(C{0.2, 0.2, true, std::numeric_limits<double>::infinity()}, 20) ==
         V::RangeOverflow);
  EXPECT(kernels::fast_form_safe<float>(C{0.2, 0.2, true, 0.0}, 32));
}

// plan_call (runtime/call_plan.hpp): the schedule of one run(iters) call.
static bool plan_is(const CallPlan& p, std::initializer_list<PlanStep> want) {
  if (p.n_steps != int(want.size())) return false;
  int i = 0;
  for (const PlanStep& w : want) {
    const PlanStep& s = p.steps[i++];
    if (s.kind != w.kind || s.S != w.S || s.count != w.count) return false;
  }
  return true;
}

static void test_call_plan() {
  using M = SuperstepMode;
  using K = StepKind;
  EXPECT(superstep_mode(true, false, true) == M::Fused);
  EXPECT(superstep_mode(false, true, true) == M::Direct);
  EXPECT(superstep_mode(false, false, true) == M::Overlap);
  EXPECT(superstep_mode(false, false, false) == M::PostExchange);
  const M modes[4] = {M::Fused, M::Direct, M::Overlap, M::PostExchange};
  const int blocks[6] = {1, 7, 16, 20, 24, 32};
  for (int iters = 0; iters <= 100; ++iters)
    for (int block : blocks)
      for (M mode : modes)
        for (int flags = 0; flags < 16; ++flags) {
          const bool multi = flags & 1, opening = flags & 2, steady = flags & 4, fresh = flags & 8;
          const CallPlan p = plan_call(iters, block, mode, multi, opening, steady, fresh);
          const bool post = mode == M::PostExchange;
          EXPECT(p.n_steps <= CallPlan::kMaxSteps && p.n_blocks <= 2);
          int sum = 0, supersteps = 0, primes = 0, bares = 0, openings = 0, lo = 1 << 30, hi = 0;
          for (int i = 0; i < p.n_steps; ++i) {
            const PlanStep& s = p.steps[i];
            EXPECT(s.count >= 1 && s.S >= 1 && s.S <= block);
            if (s.kind == K::Prime) {
              ++primes;
              continue;
            }
            sum += s.S * s.count;
            supersteps += s.count;
            lo = std::min(lo, s.S);
            hi = std::max(hi, s.S);
            if (s.kind == K::Bare) ++bares;
            if (s.kind == K::Opening) openings += s.count;
          }
          EXPECT(sum == iters);
          EXPECT(supersteps == (iters + block - 1) / block);
          EXPECT(iters == 0 || hi - lo <= 1);  // at most two sizes, differing by one
          int block_sum = 0, block_steps = 0;
          for (int i = 0; i < p.n_blocks; ++i) {
            block_sum += p.blocks[i].S * p.blocks[i].count;
            block_steps += p.blocks[i].count;
          }
          EXPECT(block_sum == iters && block_steps == supersteps);
          EXPECT(primes <= 1);
          EXPECT(bares <= 1);
          EXPECT(bares == 0 || mode == M::PostExchange || mode == M::Direct);
          EXPECT(openings == 0 || (opening && post));
          EXPECT((p.label == OpeningLabel::None) == (iters == 0));
          if (iters == 0) {
            EXPECT(p.n_steps == 0 && p.exchanges == 0);
            continue;
          }
          const K last = p.steps[p.n_steps - 1].kind;
          if (mode == M::Fused) EXPECT(p.exchanges == 0 && p.label == OpeningLabel::Fused);
          if (mode == M::Overlap) EXPECT(p.exchanges == supersteps && p.label == OpeningLabel::Overlap);
          if (mode == M::Direct) {
            EXPECT(p.exchanges == (multi ? supersteps - 1 : supersteps) + 1 && p.label == OpeningLabel::Direct);
            EXPECT((last == K::Bare) == multi);
          }
          if (post && multi) {
            // One exchange per super-step on every rank, whatever was decided. The call ends
            // on the bare pass, or on the opening where that is the last super-step too:
            // every super-step of a steady interior-first call, the only one of a short call.
            EXPECT(p.exchanges == supersteps);
            EXPECT(p.label == OpeningLabel::Primed && !p.ring_fresh);
            const bool ends_on_opening = opening && (steady || supersteps == 1);
            EXPECT(last == (ends_on_opening ? K::Opening : K::Bare));
            EXPECT(openings == (!opening ? 0 : steady ? supersteps : 1));
          }
          if (post && !multi) {
            // One rank: no bare tail; a stale ring costs one exchange more. Calls that end
            // on an opening (the steady interior-first schedule's, a stale one-super-step
            // call's) exchange every super-step's input instead and leave the ring stale.
            const bool all_openings = opening && (steady || (!fresh && supersteps == 1));
            EXPECT(bares == 0);
            EXPECT(p.exchanges == supersteps + (!all_openings && !fresh ? 1 : 0));
            EXPECT(p.ring_fresh == !all_openings);
            if (!all_openings) EXPECT(p.label == (fresh ? OpeningLabel::Fresh : OpeningLabel::Primed));
          }
        }
  // Spelled-out calls.
  CallPlan p = plan_call(20, 20, M::PostExchange, true, true, false, false);
  EXPECT(plan_is(p, {{K::Opening, 20, 1}}) && p.exchanges == 1 && p.label == OpeningLabel::Primed);
  EXPECT(p.n_blocks == 1 && p.blocks[0].S == 20 && p.blocks[0].count == 1);
  p = plan_call(240, 20, M::PostExchange, true, true, false, false);
  EXPECT(plan_is(p, {{K::Opening, 20, 1}, {K::Prime, 20, 1}, {K::Full, 20, 10}, {K::Bare, 20, 1}}) && p.exchanges == 12);
  p = plan_call(240, 20, M::PostExchange, true, true, true, false);  // steady: all openings, no bare tail
  EXPECT(plan_is(p, {{K::Opening, 20, 12}}) && p.exchanges == 12 && !p.ring_fresh);
  p = plan_call(47, 20, M::PostExchange, true, false, false, false);  // 16 + 16 + 15, the 16s first
  EXPECT(plan_is(p, {{K::Prime, 16, 1}, {K::Full, 16, 2}, {K::Bare, 15, 1}}) && p.exchanges == 3);
  EXPECT(p.n_blocks == 2 && p.blocks[0].S == 16 && p.blocks[0].count == 2 && p.blocks[1].S == 15 && p.blocks[1].count == 1);
  EXPECT(std::string(to_string(p.label, false)) == "serial");
  p = plan_call(47, 20, M::PostExchange, true, true, false, false);  // the opening takes one of the 16s
  EXPECT(plan_is(p, {{K::Opening, 16, 1}, {K::Prime, 16, 1}, {K::Full, 16, 1}, {K::Bare, 15, 1}}) && p.exchanges == 3);
  p = plan_call(31, 24, M::PostExchange, true, true, false, false);  // 16 + 15: the second group primes
  EXPECT(plan_is(p, {{K::Opening, 16, 1}, {K::Prime, 15, 1}, {K::Bare, 15, 1}}) && p.exchanges == 2);
  p = plan_call(31, 24, M::PostExchange, true, true, true, false);
  EXPECT(plan_is(p, {{K::Opening, 16, 1}, {K::Opening, 15, 1}}) && p.exchanges == 2);
  p = plan_call(30, 24, M::PostExchange, false, false, false, true);  // one rank, fresh ring
  EXPECT(plan_is(p, {{K::Full, 15, 2}}) && p.exchanges == 2 && p.label == OpeningLabel::Fresh && p.ring_fresh);
  EXPECT(std::string(to_string(p.label, true)) == "fresh");
  p = plan_call(30, 24, M::PostExchange, true, false, false, true);  // with peers a fresh ring is primed all the same
  EXPECT(plan_is(p, {{K::Prime, 15, 1}, {K::Full, 15, 1}, {K::Bare, 15, 1}}) && p.exchanges == 2);
  p = plan_call(60, 20, M::Direct, true, true, true, false);  // pushes: the priming one + all but the bare tail's
  EXPECT(plan_is(p, {{K::Full, 20, 2}, {K::Bare, 20, 1}}) && p.exchanges == 3);
  p = plan_call(60, 20, M::Fused, false, false, false, false);
  EXPECT(plan_is(p, {{K::Full, 20, 3}}) && p.exchanges == 0 && std::string(to_string(p.label, false)) == "fused");
  EXPECT(std::string(to_string(OpeningLabel::Primed, true)) == "interior-first" &&
         std::string(to_string(OpeningLabel::None, true)).empty());
  // split(): ceil(iters / block) near-equal blocks, the larger size first.
  BlockGroup g[2];
  split(20, 24, g);
  EXPECT(g[0].count == 0 && g[1].S == 20 && g[1].count == 1);
  split(30, 24, g);
  EXPECT(g[0].count == 0 && g[1].S == 15 && g[1].count == 2);
  split(47, 20, g);
  EXPECT(g[0].S == 16 && g[0].count == 2 && g[1].S == 15 && g[1].count == 1);
  split(0, 20, g);
  EXPECT(g[0].count == 0 && g[1].count == 0);
}

// A scripted device for cg_drive: runs[k] is what the scalar block reads after
// the k-th start and after each of its blocks, truths the true residuals in the
// order they are asked for.
struct CgScript {
  std::vector<std::vector<CgProgress>> runs;
  std::vector<CgResidual> truths;
  struct StartArgs {
    double tol;
    int remaining, norm_id;
  };
  std::vector<StartArgs> starts;
  int steps = 0, truths_taken = 0;
  size_t at = 0;

  CgSolve drive(double tol, int max_iters, const std::string& norm = "l2", int check_every = 2,
                const char* who = "conjugate gradients") {
    return cg_drive(
        who, tol, max_iters, norm, check_every,
        [&](double t, int remaining, int norm_id) {
          starts.push_back({t, remaining, norm_id});
          at = 0;
          return runs.at(starts.size() - 1).at(at++);
        },
        [&] {
          ++steps;
          return runs.at(starts.size() - 1).at(at++);
        },
        [&] { return truths.at(size_t(truths_taken++)); });
  }
};

static bool history_is(const CgSolve& s, std::initializer_list<CgSolve::Check> want) {
  if (s.history.size() != want.size()) return false;
  size_t i = 0;
  for (const CgSolve::Check& w : want) {
    const CgSolve::Check& h = s.history[i++];
    if (h.iteration != w.iteration || h.linf != w.linf || h.l2 != w.l2) return false;
  }
  return true;
}

template <typename F>
static std::string thrown_by(F&& f) {
  try {
    f();
  } catch (const std::invalid_argument& e) {
    return e.what();
  }
  return "(nothing thrown)";
}

static void test_cg_protocol() {
  using kernels::kCgBreakdown;
  using kernels::kCgConverged;
  using kernels::kCgMaxIters;
  using kernels::kCgRunning;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  // rr values are squares, so the history's l2 = sqrt(rr) is exact.
  {  // converged at the first read: one entry at iteration 0, the true residual reported
    CgScript s;
    s.runs = {{{kCgConverged, 0, 0.25, 0.375}}};
    s.truths = {{0.0625, 0.125, 6}};
    const CgSolve r = s.drive(1.0, 100);
    EXPECT(r.converged && r.iterations == 0 && r.restarts == 0 && r.norm == "l2");
    EXPECT(r.reason == "converged: l2 residual <= tol");
    EXPECT(r.residual == 0.125);  // the true one, not sqrt(rr) = 0.5
    EXPECT(history_is(r, {{0, 0.375, 0.5}}));
    EXPECT(s.starts.size() == 1 && s.starts[0].tol == 1.0 && s.starts[0].remaining == 100 &&
           s.starts[0].norm_id == kernels::kCgNormL2);
    EXPECT(s.steps == 0 && s.truths_taken == 1);
  }
  {  // one history entry per block after the start's; linf picks the other norm
    CgScript s;
    s.runs = {{{kCgRunning, 0, 16.0, 3.0}, {kCgRunning, 2, 4.0, 1.5}, {kCgConverged, 3, 0.25, 0.25}}};
    s.truths = {{0.3125, 0.5, 6}};
    const CgSolve r = s.drive(0.4, 100, "linf");
    EXPECT(r.converged && r.iterations == 3 && r.restarts == 0 && r.norm == "linf");
    EXPECT(r.reason == "converged: linf residual <= tol" && r.residual == 0.3125);
    EXPECT(history_is(r, {{0, 3.0, 4.0}, {2, 1.5, 2.0}, {3, 0.25, 0.5}}));
    EXPECT(s.starts[0].norm_id == kernels::kCgNormLinf && s.steps == 2 && s.truths_taken == 1);
  }
  {  // the device converged, the true residual did not: one restart, then converged
    CgScript s;
    s.runs = {{{kCgRunning, 0, 16.0, 3.0}, {kCgRunning, 2, 4.0, 1.5}, {kCgConverged, 4, 0.25, 0.25}},
              {{kCgRunning, 0, 9.0, 2.0}, {kCgConverged, 2, 0.0625, 0.125}}};
    s.truths = {{2.0, 3.0, 6}, {0.125, 0.25, 6}};
    const CgSolve r = s.drive(1.0, 10);
    EXPECT(r.converged && r.iterations == 6 && r.restarts == 1 && r.residual == 0.25);
    EXPECT(r.reason == "converged: l2 residual <= tol");
    EXPECT(history_is(r, {{0, 3.0, 4.0}, {2, 1.5, 2.0}, {4, 0.25, 0.5}, {4, 2.0, 3.0}, {6, 0.125, 0.25}}));
    EXPECT(s.starts.size() == 2 && s.starts[0].remaining == 10 && s.starts[1].remaining == 6 && s.starts[1].tol == 1.0);
    EXPECT(s.steps == 3 && s.truths_taken == 2);
  }
  {  // the same failure more than kCgMaxRestarts times: stalled
    CgScript s;
    s.runs.assign(4, {{kCgRunning, 0, 16.0, 3.0}, {kCgConverged, 2, 0.25, 0.25}});
    s.truths.assign(4, {2.0, 3.0, 6});
    const CgSolve r = s.drive(1.0, 1000);
    EXPECT(!r.converged && r.reason == "stalled" && r.restarts == 3 && kCgMaxRestarts == 3);
    EXPECT(r.iterations == 8 && r.residual == 3.0);
    EXPECT(history_is(r, {{0, 3.0, 4.0}, {2, 0.25, 0.5}, {2, 3.0, 4.0}, {4, 0.25, 0.5}, {4, 3.0, 4.0}, {6, 0.25, 0.5},
                          {6, 3.0, 4.0}, {8, 0.25, 0.5}}));
    EXPECT(s.starts.size() == 4 && s.starts[3].remaining == 994 && s.truths_taken == 4);
  }
  {  // the device converged, the true residual did not, nothing remains: no restart
    CgScript s;
    s.runs = {{{kCgRunning, 0, 16.0, 3.0}, {kCgConverged, 2, 0.25, 0.25}}};
    s.truths = {{2.0, 3.0, 6}};
    const CgSolve r = s.drive(1.0, 2);
    EXPECT(!r.converged && r.reason == "max_iters reached" && r.restarts == 0 && r.iterations == 2 && r.residual == 3.0);
    EXPECT(history_is(r, {{0, 3.0, 4.0}, {2, 0.25, 0.5}}));
    EXPECT(s.starts.size() == 1 && s.truths_taken == 1);
  }
  {  // the device ran out of iterations: the true residual once, at the end
    CgScript s;
    s.runs = {{{kCgRunning, 0, 16.0, 3.0}, {kCgRunning, 2, 9.0, 2.0}, {kCgMaxIters, 4, 4.0, 1.0}}};
    s.truths = {{1.5, 2.5, 6}};
    const CgSolve r = s.drive(1.0, 4);
    EXPECT(!r.converged && r.reason == "max_iters reached" && r.restarts == 0 && r.iterations == 4 && r.residual == 2.5);
    EXPECT(history_is(r, {{0, 3.0, 4.0}, {2, 2.0, 3.0}, {4, 1.0, 2.0}}));
    EXPECT(s.starts.size() == 1 && s.steps == 2 && s.truths_taken == 1);
  }
  {  // p . L p not positive, the residual finite
    CgScript s;
    s.runs = {{{kCgRunning, 0, 16.0, 3.0}, {kCgBreakdown, 1, 9.0, 2.0}}};
    s.truths = {{1.5, 2.5, 6}};
    const CgSolve r = s.drive(1.0, 50);
    EXPECT(!r.converged && r.reason == "breakdown" && r.iterations == 1 && r.residual == 2.5 && r.restarts == 0);
    EXPECT(history_is(r, {{0, 3.0, 4.0}, {1, 2.0, 3.0}}));
    EXPECT(s.truths_taken == 1);
  }
  {  // the same status with a NaN rr, and with a NaN linf
    CgScript s;
    s.runs = {{{kCgRunning, 0, 16.0, 3.0}, {kCgBreakdown, 1, nan, 2.0}}};
    s.truths = {{nan, nan, 6}};
    CgSolve r = s.drive(1.0, 50);
    EXPECT(!r.converged && r.reason == "non-finite residual" && r.iterations == 1 && std::isnan(r.residual));
    EXPECT(r.history.size() == 2 && r.history[1].iteration == 1 && r.history[1].linf == 2.0 && std::isnan(r.history[1].l2));
    CgScript t;
    t.runs = {{{kCgBreakdown, 0, 4.0, nan}}};
    t.truths = {{1.0, 1.0, 6}};
    r = t.drive(1.0, 50);
    EXPECT(!r.converged && r.reason == "non-finite residual" && t.steps == 0);
  }
  {  // a reported convergence whose true residual is not finite (either norm's)
    CgScript s;
    s.runs = {{{kCgConverged, 0, 0.25, 0.25}}};
    s.truths = {{0.5, nan, 6}};
    CgSolve r = s.drive(1.0, 50);
    EXPECT(!r.converged && r.reason == "non-finite residual" && r.restarts == 0 && std::isnan(r.residual));
    EXPECT(s.starts.size() == 1 && s.truths_taken == 1);
    CgScript t;
    t.runs = {{{kCgConverged, 0, 0.25, 0.25}}};
    t.truths = {{nan, 0.5, 6}};
    r = t.drive(1.0, 50);  // l2 is finite and below tol, linf is not finite
    EXPECT(!r.converged && r.reason == "non-finite residual" && r.residual == 0.5);
  }
  {  // max_iters == 0: the start kernel runs (it reports kCgMaxIters), no block does
    CgScript s;
    s.runs = {{{kCgMaxIters, 0, 16.0, 3.0}}};
    s.truths = {{3.0, 4.0, 6}};
    const CgSolve r = s.drive(1.0, 0);
    EXPECT(!r.converged && r.reason == "max_iters reached" && r.iterations == 0 && r.residual == 4.0);
    EXPECT(history_is(r, {{0, 3.0, 4.0}}));
    EXPECT(s.starts.size() == 1 && s.starts[0].remaining == 0 && s.steps == 0 && s.truths_taken == 1);
  }
  {  // bad arguments: invalid_argument with the solver's prefix, nothing launched
    CgScript s;
    EXPECT(thrown_by([&] { s.drive(1.0, 10, "l1"); }) == "conjugate gradients: norm must be 'linf' or 'l2', got 'l1'");
    EXPECT(thrown_by([&] { s.drive(1.0, 10, "l1", 2, "preconditioned CG"); }) ==
           "preconditioned CG: norm must be 'linf' or 'l2', got 'l1'");
    const std::string args = ": solve needs tol >= 0, max_iters >= 0 and check_every >= 1";
    EXPECT(thrown_by([&] { s.drive(nan, 10); }) == "conjugate gradients" + args);
    EXPECT(thrown_by([&] { s.drive(-1e-9, 10); }) == "conjugate gradients" + args);
    EXPECT(thrown_by([&] { s.drive(1.0, -1); }) == "conjugate gradients" + args);
    EXPECT(thrown_by([&] { s.drive(1.0, 10, "l2", 0); }) == "conjugate gradients" + args);
    EXPECT(thrown_by([&] { s.drive(1.0, 10, "linf", 0, "preconditioned CG"); }) == "preconditioned CG" + args);
    EXPECT(s.starts.empty() && s.steps == 0 && s.truths_taken == 0);
  }
}

int main() {
  test_cg_protocol();
  test_call_plan();
  test_pipe_form();
  test_fast_form_verdict();
  test_regions();
  test_layout();
  test_cart();
  test_plan();
  test_decision();
  test_halo_last_schedule();
  if (g_failures) {
    std::fprintf(stderr, "%d failure(s)\n", g_failures);
    return 1;
  }
  std::printf("mxs_unit_tests: all passed\n");
  return 0;
}
