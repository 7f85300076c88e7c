// Which stream every chain of a forward runs on and which events order them: decided ONCE, before the first launch, from the switches
// and the per-call facts below.  forward_impl (engine.hip) and rift_forward's arena-poison fill read nothing else for a stream
// selection, an event record or a stream wait.  Host-only and free of HIP, so that tests/test_host_api.py can compile it with the system
// compiler and check every combination of the inputs.
//
// The chains: the input preparation; the agent-history chain (NAT levels + FPN tail); the map chain (ego token, PointsEncoders, Fourier
// embeddings, decoder queries); the caller's token assembly -> encoder -> decoder.  History and map chain depend on the preparation only
// and join at the token assembly.
//
// With the preparation prefetched, neither front chain of step k + 1 needs anything of step k: the map chain (side stream) waits for
// the preparation only, the agent-history chain follows it on the prepare stream, and the caller's queue holds token assembly ->
// encoder -> decoder of step k, then of step k + 1 -- the fronts run beside the previous step's one-workgroup-per-scene encoder /
// decoder (which leave most of the chip idle below 256 scenes; at 256 they hold every CU whole, and what is gained is that the fronts
// start the moment CUs come free, with gather and preparation long done -- profiles/r03_timeline_256.txt).  ms per step, fronts behind the caller's queue
// / beside it: 32 scenes 0.372 / 0.237, 64 0.394 / 0.245, 128 0.462 / 0.389, 192 0.597 / 0.524, 256 0.701 / 0.678.  What it took:
// RIFT_DEFER_SLOTS = 4 arenas (with two, tail k - 1 -> front k + 1 -> encoder / decoder k + 1 -> tail k + 1 is a cycle two steps long)
// and no further hardware queue for the history chain (on a stream of its own every cross-queue wait of the step got slower: 0.372).
#pragma once

enum PlanStream { ON_CALLER = 0, ON_PREPARE = 1, ON_SIDE = 2 };      // the caller's stream, the caller's prepare stream, the engine's side stream

struct PlanIn {
  bool two_streams, nat_fused, nat_aside; int side_gate;     // switches (RIFT_TWO_STREAMS, RIFT_NAT_UNFUSED, RIFT_NAT_ASIDE, RIFT_SIDE_GATE)
  bool fp32, prof_on, dry, prep_set, dp_on; int bs;          // per call (prep_set: rift_set_prepare_stream, dp_on: rift_set_dp)
};

struct StreamPlan {
  bool prefetched;        // the preparation runs on the caller's prepare stream, which records ev_prep behind it
  bool forked;            // history and map chains run on two streams; the side stream records ev_join behind the map chain and the caller waits for it
  bool nat_aside;         // the history chain follows the preparation on the prepare stream, which records ev_join2 behind it
  PlanStream prep_on, history_on, map_on, dp_fill_on;
  bool dp_fill_late;      // data parallel: the mask fill behind the history chain's hand-back (on dp_fill_on) instead of right behind the preparation
  bool side_waits_prep;   // the side stream waits for ev_prep
  bool fork_from_main;    // the caller's stream records ev_fork and the side stream waits for it
  bool main_waits_prep;   // the caller's stream waits for ev_prep right behind the preparation
  bool join_once;         // the side stream waits for ev_join2 ahead of its ev_join record; otherwise the caller's stream waits for ev_join2 itself
};

inline StreamPlan plan_streams(const PlanIn& in) {
  StreamPlan p;
  // the prepare stream is the caller's: behind the gather of the batch, beside the previous step.  Off while profiling per kernel.
  p.prefetched = in.prep_set && !in.prof_on && !in.dry;
  // fork: on its own stream each chain fills the CUs the other leaves idle (partial last rounds, 238-workgroup launches)
  p.forked = in.two_streams && in.nat_fused && !in.fp32 && !in.prof_on && !in.dry;
  // RIFT_SIDE_GATE=1 keeps both fronts behind the caller's queue (the event record costs that queue ~5 us), RIFT_NAT_ASIDE=0 the history chain on it
  const bool gate = in.side_gate > 0;
  p.nat_aside = p.forked && p.prefetched && !gate && in.nat_aside;
  p.prep_on = p.prefetched ? ON_PREPARE : ON_CALLER;
  // the longer chain (agent history: ~310 of the front's ~510 us at 256 scenes) never takes a queue of its own, so neither its start nor
  // the join pays a cross-queue hop (12-15 us each by the kernel trace); the map / reference-line chain is the one that forks
  p.history_on = p.nat_aside ? ON_PREPARE : ON_CALLER;
  p.map_on = p.forked ? ON_SIDE : ON_CALLER;
  // (with the preparation prefetched the fill waits for the head of the map chain: the exchange buffer is the one the previous forward's
  // map chain exchanged through, and that chain's stream is what orders the two)
  p.dp_fill_late = in.dp_on && p.prefetched;
  p.dp_fill_on = p.dp_fill_late ? p.map_on : ON_CALLER;
  p.side_waits_prep = p.forked && p.prefetched;
  p.fork_from_main = p.forked && (!p.prefetched || gate);
  // When the history chain stays on the prepare stream and the map chain forks onto the side stream (the update loop's case), the caller's
  // queue gets nothing before the join, and both joined chains are behind the preparation already: its own wait would be a third one on
  // the same fact (one event operation costs the host what a launch does)
  p.main_waits_prep = p.prefetched && !(p.forked && p.nat_aside && !in.dp_on);
  // Small batches: the map chain waits for the history chain first, so that the caller's queue -- token assembly, encoder, decoder: the
  // step, below a chip-filling batch -- takes ONE cross-queue wait per forward (32 scenes: 0.233 -> 0.226 ms); at 128 scenes it makes no
  // difference and at 256 it costs 1-3 % (the map chain of the step after next stalls behind the wait)
  p.join_once = p.nat_aside && in.bs <= 64;
  return p;
}
