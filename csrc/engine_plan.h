// What an epoch launches (host only, csrc/engine.cpp): the DLAP_* switches, the per-phase launch
// plan derived from them, and the arguments of one training / evaluation pass.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

// Per-model workgroups of a tower launch over G batched models (grid.y = model): the single-
// model grid tuned at 600x3000 (`one`) divided by G, at least `lo`. The whole launch then keeps
// roughly the single-model workgroup count instead of G times it: fewer weight stagings per
// row and, in the backward, G-fold fewer gradient slabs for k_finalize to reduce. Measured
// (profiles/r3_knobs_grids_batched.log): 9 models 1.045 -> 0.823 ms per epoch, 2 models
// 0.337 -> 0.271 ms.
inline int grid_per_model(int one, int lo, int G) { return std::max(lo, one / std::max(1, G)); }

inline int env_int(const char* name, int dflt) {
  const char* v = std::getenv(name);
  return v && *v ? std::atoi(v) : dflt;
}

// Every DLAP_* switch the engine runtime reads, latched ONCE when an engine is constructed
// (read_knobs): set the variables before building the engine, later changes of the environment
// are not seen. Safe mode (Engine::set_safe_mode) is an overlay on these values, not a re-read.
struct Knobs {
  // ---- which pipeline runs
  bool rnn_overlap;        // DLAP_RNN_OVERLAP (1): fused LSTM + training tower forward (k_mlp_fwd_rnn)
  bool rnn_overlap_eval;   // DLAP_RNN_OVERLAP_EVAL (0): ... also for an evaluation beside the training chain
  bool fused_p2;           // DLAP_FUSED_PHASE2 (0): fused training forward in phase 2 too
  bool eval_in_fwd;        // DLAP_EVAL_IN_FWD (1): evaluation recurrences inside the fused training forward
  bool eval_sep;           // DLAP_EVAL_SEP (0): evaluation recurrences on the evaluation queue (split graphs)
  bool self_proj;          // DLAP_SELF_PROJ (1): the fused launch's recurrences project their own inputs
  bool fused_tail;         // DLAP_FUSED_TAIL (1): k_finalize -> k_lstm_bwd -> k_wgrad as one launch (k_lstm_tail)
  bool mom_tail;           // DLAP_MOM_TAIL (1): phase 2's finalize + wgrad + Adam + metrics as one launch
  int tail_adam;           // DLAP_TAIL_ADAM (1): clip + Adam in the tail; 2: also in the one-graph fallback
  bool split_graphs;       // DLAP_SPLIT_GRAPHS (1): training chain and evaluation as two graphs
  int unroll;              // DLAP_UNROLL (8): body epochs per split-graph launch
  bool p2_lstm_cache;      // DLAP_P2_LSTM_CACHE (1): phase 2's LSTM recurrence once per run_epochs call
  bool train_gram_side;    // DLAP_TRAIN_GRAM_SIDE (0): phase-start train Gram build on the evaluation stream
  bool h_cache;            // DLAP_H_CACHE (1): moments cached while the moment network is frozen
  bool gram;               // DLAP_GRAM (1): Gram-form losses (k_gram.hip)
  int gram_plan;           // DLAP_GRAM_PLAN (1): per-phase cost model; 0 Gram wherever it applies,
                           //   2 dense evaluation splits, 3 dense train split
  bool fused_pack;         // DLAP_FUSED_PACK (1): k_adam re-packs through per-parameter scatter lists
  int tail_masks;          // DLAP_TAIL_MASKS (1): split graphs of one model, the next step's keep words from
                           //   blocks of the tail launch instead of k_dropmask on the evaluation queue (> 1:
                           //   that many mask blocks per model at any batch size, for tests and measurements)
  // ---- in-kernel waits, co-residency
  int prog_mode;           // DLAP_PROG_MODE (1): see MlpJob::prog_mode
  unsigned spin_limit;     // DLAP_PROG_SPIN_LIMIT (1 << 22): polls before a wait gives up (safe mode raises
                           //   it to at least the default, for good)
  int fused_cap;           // DLAP_FUSED_CAP (-1): >= 0 overrides the fused launches' co-residency capacity
  // ---- model descriptor
  bool wide;               // DLAP_WIDE (0): force the streaming layer-0 path
  int tps;                 // DLAP_TPS (1): 2 = two gradient tiles per slice of the sliced backward
  bool tbwd;               // DLAP_TBWD (1): one-pass SDF tower backward (k_tbwd.hip)
  // ---- grids and partitions
  int eval_gx;             // DLAP_EVAL_GX (256 / G, >= 64): cap on the evaluation tower grid per job
  bool zx_eval, zx_train;  // DLAP_ZX_EVAL / DLAP_ZX_TRAIN (1): wide path, layer 0 fused into the towers (bf16 only)
  int zx_gx;               // DLAP_ZX_GX (256): their workgroups over all jobs of a launch
  int gx_fwd;              // DLAP_GX_FWD (1024; G > 2: 1024 / G, >= 128): tower forward grid per model
  int gx_fwd13;            // DLAP_GX_FWD13 (384 / G, >= 96): training forward grid of phases 1 / 3
  int gx_proj;             // DLAP_GX_PROJ (512): wide path, k_proj0 grid
  int wg_split;            // DLAP_WG_SPLIT (512): wide path, split-K of the layer-0 weight gradient
  int nslab_coarse;        // DLAP_NSLAB_COARSE (64): coarse backward slabs per model (4 fine slabs each)
  int bwd_fpw;             // DLAP_BWD_FPW (1): 4 = four fine slabs per backward workgroup
  bool pp_global;          // DLAP_PP_GLOBAL (0): per-period tower inputs from global memory, not LDS
};

inline Knobs read_knobs(int G, bool fp32) {
  Knobs k{};
  k.rnn_overlap = env_int("DLAP_RNN_OVERLAP", 1) != 0;
  k.rnn_overlap_eval = env_int("DLAP_RNN_OVERLAP_EVAL", 0) != 0;
  k.fused_p2 = env_int("DLAP_FUSED_PHASE2", 0) != 0;
  k.eval_in_fwd = env_int("DLAP_EVAL_IN_FWD", 1) != 0;
  k.eval_sep = env_int("DLAP_EVAL_SEP", 0) != 0;
  k.self_proj = env_int("DLAP_SELF_PROJ", 1) != 0;
  k.fused_tail = env_int("DLAP_FUSED_TAIL", 1) != 0;
  k.mom_tail = env_int("DLAP_MOM_TAIL", 1) != 0;
  k.tail_adam = env_int("DLAP_TAIL_ADAM", 1);
  k.split_graphs = env_int("DLAP_SPLIT_GRAPHS", 1) != 0;
  k.unroll = std::max(1, env_int("DLAP_UNROLL", 8));
  k.p2_lstm_cache = env_int("DLAP_P2_LSTM_CACHE", 1) != 0;
  k.train_gram_side = env_int("DLAP_TRAIN_GRAM_SIDE", 0) != 0;
  k.h_cache = env_int("DLAP_H_CACHE", 1) != 0;
  k.gram = env_int("DLAP_GRAM", 1) != 0;
  k.gram_plan = env_int("DLAP_GRAM_PLAN", 1);
  k.fused_pack = env_int("DLAP_FUSED_PACK", 1) != 0;
  k.tail_masks = std::max(0, env_int("DLAP_TAIL_MASKS", 1));
  k.prog_mode = env_int("DLAP_PROG_MODE", 1);
  k.spin_limit = (unsigned)env_int("DLAP_PROG_SPIN_LIMIT", 1 << 22);
  k.fused_cap = env_int("DLAP_FUSED_CAP", -1);
  k.wide = env_int("DLAP_WIDE", 0) != 0;
  k.tps = env_int("DLAP_TPS", 1);
  k.tbwd = env_int("DLAP_TBWD", 1) != 0;
  // evaluation tower grid cap: with the split epoch graphs the evaluation branch has slack and
  // its towers start beside the training chain's loss passes; a narrower grid takes fewer CUs
  // from them -- 224-256 measured best (phase 3 0.1554 vs 0.164 ms at 384, profiles/
  // r5_knobs_eval_gx.log; 384 was best on the round-3 tree). Per job: with G batched models the
  // launch has 2G evaluation jobs, so the per-job grid shrinks with G (see grid_per_model)
  k.eval_gx = env_int("DLAP_EVAL_GX", grid_per_model(256, 64, G));
  // fp32 wide path: layer 0 through k_proj0 + the ZIN towers (the fused-layer-0 k_mlp_fwd_zx
  // is bf16 only)
  k.zx_eval = !fp32 && env_int("DLAP_ZX_EVAL", 1) != 0;
  k.zx_train = !fp32 && env_int("DLAP_ZX_TRAIN", 1) != 0;
  k.zx_gx = std::max(1, env_int("DLAP_ZX_GX", 256));
  // tower-forward grids (measured, 600x3000x46 epoch graph): the phase-1/3 training forward
  // runs SDF-only (moments cached) beside the evaluation branch and is fastest with one
  // workgroup per CU (256); phase 2 (moment tower, no evaluation branch) with 1024
  k.gx_fwd = env_int("DLAP_GX_FWD", G <= 2 ? 1024 : grid_per_model(1024, 128, G));
  k.gx_fwd13 = env_int("DLAP_GX_FWD13", grid_per_model(384, 96, G));
  k.gx_proj = env_int("DLAP_GX_PROJ", 512);
  k.wg_split = env_int("DLAP_WG_SPLIT", 512);
  k.nslab_coarse = env_int("DLAP_NSLAB_COARSE", 64);
  k.bwd_fpw = env_int("DLAP_BWD_FPW", 1);
  k.pp_global = env_int("DLAP_PP_GLOBAL", 0) != 0;
  return k;
}

// The launch plan of one phase (1..3), computed by Engine::rebuild_jobs once the co-residency
// capacities are known. Its inputs -- the knobs, the model descriptor, the split sizes, the
// capacities, sharding, the re-pack lists and safe mode -- change only together with a rebuild.
// Engine::set_pipeline does not rebuild: run_mode() combines the plan with it.
struct PhasePlan {
  bool fused_fwd = false;       // fused LSTM + training tower forward ...
  int train_gx = 0;             // ... and its capped grid (0: two launches)
  bool eval_in_fwd = false;     // evaluation recurrences ride in the fused training forward ...
  int all_gx = 0;               // ... whose capped grid is then this
  bool selfproj = false;        // the fused training forward's recurrences project their own inputs
  bool sep_eval = false;        // split graphs with the evaluation recurrences on the evaluation queue
  bool tail_fused = false;      // backward tail as one launch (k_lstm_tail)
  bool adam_in_tail = false;    // the tail may carry the clip + Adam update (co-residency guard passed)
  bool split_graphs = false;    // training chain and evaluation as two graphs
  bool tail_masks = false;      // ... whose tail launch hashes the next step's keep words (no k_dropmask on
  int mask_blocks = 0;          //     the evaluation queue), in this many more blocks per model
  bool mom_tail = false;        // phase 2: the moment network's one-launch tail
  bool p2_lstm_cached = false;  // phase 2: the LSTM recurrence once per run
  bool eval_fusable = false;    // an evaluation on its own may run the fused LSTM + tower launch ...
  int eval_gx_solo = 0;         // ... on this capped grid
};

// How run_epochs runs a phase: the plan combined with set_pipeline (also what fused_info reports)
struct RunMode {
  bool pipe = false;            // software-pipelined epochs: head | body x (n-1) | tail
  bool split = false;           // ... body as the two split graphs
  bool sep = false;             // ... with the evaluation recurrences on the evaluation queue
  bool tail_adam = false;       // the body's update runs in the backward tail (no k_adam launch)
};

// One training pass (masks -> forward -> losses -> tower backward -> tail) of the train split
struct TrainPass {
  explicit TrainPass(int phase_, float lr_ = 0.f) : phase(phase_), lr(lr_) {}
  int phase;
  float lr;                     // learning rate of an update inside the tail (tail_adam / mom_adam)
  bool gram = false;            // Gram-form loss (epoch graphs, where the plan says so); dense else
  int part = 0;                 // 0: the whole pass; 1: the forward only; 2: the rest (the head epoch
                                //   split around the wait for a deferred train Gram build)
  bool premasked = false;       // this step's keep masks were generated by the previous epoch graph
  bool own_proj = true;         // the recurrences may project their own inputs (PhasePlan::selfproj)
  bool eval_rnn = false;        // the evaluation splits' projections and recurrences ride in the
                                //   training prologue and fused forward ...
  int* esig = nullptr;          // ... and count here when done (split graphs' evaluation graph waits)
  hipStream_t eval_prologue = nullptr;  // the evaluation branch's LSTM prologue goes to this stream right
                                //   behind the training one (its serial recurrence starts at the epoch start)
  bool lstm_once = false;       // phase 2: the recurrence ran once before the epochs, project only
  bool mark_fwd = false;        // record EV_FWD after the tower forward (the evaluation branch forks there)
  bool defer_metrics = false;   // the caller runs the train metrics (EV_MID is recorded after the loss pass)
  bool tail_metrics = false;    // the train metrics run in the backward tail
  int tail_adam = 0;            // the update runs in the fused tail (launch_lstm_tail's adam mode), 0: not
  bool tail_masks = false;      // ... and the tail's mask blocks write the next step's keep words
  bool mom_adam = false;        // phase 2: metrics + Adam in the moment network's tail launch
};

// One evaluation pass (prologue -> towers -> losses -> metrics) of the valid / test splits
struct EvalPass {
  bool gram = false;            // Gram-form losses (epoch graphs, where the plan says so)
  bool solo = false;            // runs alone on the GPU (the pipeline's tail, the sequential epoch): fused
                                //   in any case -- beside the training chain the spinning tower workgroups of
                                //   both fused launches compete for the same CUs (profiles/r3_knobs_fused_eval.log)
  bool sep = false;             // the split graphs' evaluation graph running its own recurrences (fused)
  bool selfproj = false;        // its recurrences project their own inputs (no k_proj launch)
};
