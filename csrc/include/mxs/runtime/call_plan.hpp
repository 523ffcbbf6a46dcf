// The schedule of one StencilSolver::run(iters) call, computed before anything
// is enqueued (host only, no HIP): which steps the call consists of, how many
// halo exchanges it issues and what its opening is called.
//
// This is the statement of the solver's collective invariant: every rank must
// issue the same exchanges in the same order, whatever it decides locally.
// plan_call() therefore takes only values that are the same on every rank
// (the call's length, the agreed time block, the super-step mode, the agreed
// opening and steady decisions) plus the ring's freshness, which with peers
// is overridden (every call primes). Nothing rank-local enters: not whether
// this rank's tile has a chunk-list form at a depth, not field_changed(). A
// rank without the form runs an Opening step as exchange + bare pass, the same
// one exchange (StencilSolver::enqueue_opening), so the plan is unchanged.
#pragma once

namespace mxs {

// How a super-step (cur -> nxt) relates to its halo exchange.
enum class SuperstepMode : int {
  Fused,         // 1x1 periodic grid: the pass wraps around, no exchange at all
  Direct,        // device-initiated push: wait, pass, push of the output
  Overlap,       // thin strips: the exchange of cur under the interior
  PostExchange,  // the pass, then the exchange of its output (cur's ring must be fresh)
};

inline SuperstepMode superstep_mode(bool fused, bool direct_on, bool overlap) {
  if (fused) return SuperstepMode::Fused;
  if (direct_on) return SuperstepMode::Direct;
  return overlap ? SuperstepMode::Overlap : SuperstepMode::PostExchange;
}

// `count` super-steps of S iterations each.
struct BlockGroup {
  int S = 0, count = 0;
};

// (size, count) groups of a call of `iters` iterations: ceil(iters / block)
// near-equal blocks, the larger size first.
inline void split(int iters, int block, BlockGroup out[2]) {
  out[0] = out[1] = BlockGroup{0, 0};
  if (iters <= 0) return;
  const int blocks = (iters + block - 1) / block;
  const int base = iters / blocks, extra = iters % blocks;  // extra blocks of base + 1
  out[0] = BlockGroup{base + 1, extra};
  out[1] = BlockGroup{base, blocks - extra};
}

enum class StepKind : int {
  Opening,  // one exchange of cur's ring + one pass, `count` times: interior-first where the
            // rank has the form, else exchange + bare pass
  Prime,    // one exchange of cur's ring
  Full,     // `count` super-steps with their own exchange (graph replay, then eager)
  Bare,     // one pass without an exchange
};

struct PlanStep {
  StepKind kind = StepKind::Bare;
  int S = 0;      // depth of the step's pass (Prime: of the pass it feeds)
  int count = 0;  // Opening / Full: super-steps; Prime / Bare: 1
};

// The mode-level name of a call's opening. Primed: the call starts with an
// exchange of cur's ring; the executor resolves it to "interior-first" or
// "serial" from the rank's form at the first step's depth.
enum class OpeningLabel : int { None, Fused, Direct, Overlap, Fresh, Primed };

inline const char* to_string(OpeningLabel l, bool interior_first) {
  switch (l) {
    case OpeningLabel::Fused: return "fused";
    case OpeningLabel::Direct: return "direct";
    case OpeningLabel::Overlap: return "overlap";
    case OpeningLabel::Fresh: return "fresh";
    case OpeningLabel::Primed: return interior_first ? "interior-first" : "serial";
    default: return "";
  }
}

struct CallPlan {
  // Opening, Prime, Full, Full, Bare is the longest call.
  static constexpr int kMaxSteps = 6;
  PlanStep steps[kMaxSteps];
  int n_steps = 0;
  BlockGroup blocks[2];  // the non-empty groups of split(), in order
  int n_blocks = 0;
  // Halo exchanges the call issues, the priming one included (Direct: pushes).
  int exchanges = 0;
  OpeningLabel label = OpeningLabel::None;
  bool ring_fresh = false;  // cur's ghost ring after the call

  void add(StepKind kind, int S, int count) { steps[n_steps++] = PlanStep{kind, S, count}; }
};

// The steps of run(iters). `opening_on`: a call that starts with a priming
// exchange opens interior-first; `steady_on`: with the opening on, so does
// every later super-step. With peers (`multi_rank`) every call primes, whatever
// the rank believes about its ring, and the call's last super-step is a bare
// pass: its exchange would only feed the next call, which primes anyway, so n
// super-steps issue exactly n exchanges.
inline CallPlan plan_call(int iters, int block, SuperstepMode mode, bool multi_rank, bool opening_on, bool steady_on,
                          bool ghost_fresh) {
  CallPlan p;
  p.ring_fresh = ghost_fresh && !multi_rank;
  if (iters <= 0) return p;
  const bool post = mode == SuperstepMode::PostExchange;
  if (mode == SuperstepMode::Fused) p.label = OpeningLabel::Fused;
  if (mode == SuperstepMode::Direct) p.label = OpeningLabel::Direct;
  BlockGroup gr[2];
  split(iters, block, gr);
  bool first = true;  // the call's first non-empty group
  for (int k = 0; k < 2; ++k) {
    int count = gr[k].count;
    const int S = gr[k].S;
    if (count <= 0) continue;
    p.blocks[p.n_blocks++] = gr[k];
    const bool was_first = first;
    first = false;
    // Steady interior-first: every super-step exchanges its own input under
    // the core chunks, the first exchange being the priming one.
    if (steady_on && opening_on && post) {
      if (was_first) p.label = OpeningLabel::Primed;
      p.add(StepKind::Opening, S, count);
      p.exchanges += count;
      p.ring_fresh = false;
      continue;
    }
    // The call's first super-step takes the priming exchange as its opening.
    // Its output's ring is stale: primed by the next super-step or call.
    if (was_first && opening_on && post && !p.ring_fresh) {
      p.label = OpeningLabel::Primed;
      p.add(StepKind::Opening, S, 1);
      ++p.exchanges;
      if (--count == 0) continue;
    }
    // Post-exchange super-steps need cur's ring fresh before the first one;
    // each leaves the next one's fresh.
    if (post && !p.ring_fresh) {
      if (was_first && p.label == OpeningLabel::None) p.label = OpeningLabel::Primed;
      p.add(StepKind::Prime, S, 1);
      ++p.exchanges;
    }
    if (was_first && p.label == OpeningLabel::None) p.label = post ? OpeningLabel::Fresh : OpeningLabel::Overlap;
    // The bare tail: the last group's last super-step with peers. The direct
    // halo's last push would only feed the next call too, which primes again.
    const bool last_bare = multi_rank && k == 1 && (post || mode == SuperstepMode::Direct);
    const int full = last_bare ? count - 1 : count;
    if (mode == SuperstepMode::Direct) p.exchanges += full + (was_first ? 1 : 0);  // the priming push included
    else if (mode != SuperstepMode::Fused) p.exchanges += full;
    if (full > 0) p.add(StepKind::Full, S, full);
    if (last_bare) p.add(StepKind::Bare, S, 1);
    p.ring_fresh = post && !last_bare;
  }
  return p;
}

}  // namespace mxs
