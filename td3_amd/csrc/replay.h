// HBM-resident replay ring (device side of my_replay_buffer.ReplayBuffer_*).
#pragma once
#include "common.h"

namespace td3 {

// One transition = one AoS record of `rec` floats in HBM:
//   [ state(sd) | action(ad) | next_state(sd) | reward | not_done | pad to 16 B ]
// (the reference keeps 5 float64 SoA arrays, my_replay_buffer.py:81-85; one
// record per row makes the sample gather one contiguous read per index).
// TD3_particles rings (ReplayBuffer_particles, my_replay_buffer.py:6-69) use the record
//   [ features(F) | particles(N*D) | action(A) | next_features(F) | next_particles(N*D) |
//     reward | not_done | pad ]
// with sd = F, ad = A; the learner's encoder reads the particle blocks in place (no gather).
// Either record is an ordered list of fields, Ring::field: the arrays of the kind's rb_add* /
// rb_sample* calls in argument order, one behind the other from column 0, reward and done (stored
// as not_done = 1 - done) last.  The host packing, the stand-alone sample and the particle device
// add walk that table; the o_* names are the same offsets for the code that wants one field.
struct RingField {
  int off, len;                    // record columns [off, off + len)
};
constexpr int kRingFields = 7;
constexpr int kMaxNstep = 8;       // longest n-step horizon (rb_nstep::n)

// Optional per-row priorities (rb_enable_priorities): a 64-ary sum tree outside the records.  Level 0
// is one fp32 leaf per ring row, level l + 1 one fp32 per 64 nodes of level l; every level is padded
// with zeros to a multiple of 64, and the top level is a single group of 64 (the root group).  The
// radix is the wave width: the children of a node are one 256-byte load, and one wave finds the
// child that holds a mass with a scan across its lanes.  A node is the scan sum (pri_group_sum,
// replay.hip) of its 64 children as last recomputed -- never a running total of deltas; the total
// mass is the same sum over the root group, which every draw loads as its first step anyway.
constexpr int kMaxPriLevels = 8;   // 64^8 rows
struct PriTree {
  bool on = false;
  double alpha = 0.0, eps = 0.0;
  int levels = 0;
  float* base = nullptr;                 // the levels one behind the other
  float* level[kMaxPriLevels] = {};      // level[l]: len[l] floats (a multiple of 64)
  int64_t len[kMaxPriLevels] = {};
  float* d_max = nullptr;                // device scalar max_priority (raised by atomicMax on its bits)
};

struct Ring {
  uint64_t gen = 0;                // unique per allocation: captured graphs bake this ring in
  int sd = 0, ad = 0;
  int rec = 0;
  RingField field[kRingFields] = {};
  int nfield = 0;                  // 5 (featured) or 7 (particles)
  int o_s = 0, o_a = 0, o_s2 = 0, o_r = 0, o_nd = 0;
  int particles = 0, N = 0, D = 0;  // particle rings only
  int o_p = 0, o_p2 = 0;
  int64_t cap = 0;
  int64_t ptr = 0, size = 0;       // host mirror of my_replay_buffer.py:76-77
  float* data = nullptr;           // [cap][rec]
  int64_t* d_size = nullptr;       // device copy of `size` (read by graph-replayed sample)
  uint64_t seed = 0;
  uint64_t sample_calls = 0;       // Philox counter of the stand-alone sample()
  int device = 0;
  hipStream_t stream = nullptr;
  float* stage[2] = {nullptr, nullptr};     // pinned host staging for large adds, double-buffered
  float* stage_dev[2] = {nullptr, nullptr}; // their device addresses
  size_t stage_cap[2] = {0, 0};
  hipEvent_t stage_buf_ev[2] = {nullptr, nullptr};  // the write out of stage[i] finished
  int stage_cur = 0;
  // Ordering between the streams that read (a learner step, a stand-alone sample) and write
  // (adds, fills) the ring, recorded lazily: an access only notes its stream; an access on ANOTHER
  // stream records an event on the noted stream at that moment (covering everything queued there
  // so far) and waits on it.  Accesses on one stream need nothing (stream order), so a learner
  // that also flushes the adds on its own stream records no event per step -- a record is a
  // marker packet that drains the queue: ~4 us of GPU time per step (C2 9.60k vs 9.97k steps/s).
  // Readers are chained (a reader on a new stream waits on the previous one's), so the last
  // read stream covers them all; writes likewise.
  hipStream_t read_stream = nullptr, write_stream = nullptr;
  bool reads_pending = false, writes_pending = false;
  // the stream already ordered after the current reads / writes (nothing to wait for again)
  hipStream_t reads_seen_by = nullptr, writes_seen_by = nullptr;
  hipEvent_t read_ev = nullptr, write_ev = nullptr;
  int64_t* d_idx = nullptr;        // last drawn indices (rows) of sample()
  int idx_cap = 0;
  // The n-step lane (rb_add_device_nstep / rb_add_particles_device_nstep): the ring row of row 0 of
  // the last ns_nhist n-step ticks, most recent first, and the (rows, n, gamma) they were stored with.
  // Every other write of the ring ends the lane (ns_nhist = 0); the rows it leaves are valid
  // shorter-horizon transitions.  ns_age[0] is read, ns_age[1] written by the next tick, then they swap.
  int64_t ns_hist[kMaxNstep - 1] = {};
  int ns_nhist = 0;
  int64_t ns_rows = 0;
  int ns_n = 0;
  double ns_gamma = 0.0;
  int* ns_age[2] = {nullptr, nullptr};   // device [ns_age_rows]: ticks of this environment's episode still maturing
  int64_t ns_age_rows = 0;
  PriTree pri;
  // Dataset normalisation (ringnorm.hip; include/td3.h "dataset normalisation"): set by
  // rb_normalize_states, cleared by rb_write_records and rb_fill_synthetic, left by the adds.
  int normalized = 0;
  int64_t norm_rows = 0;           // the rows that call rewrote
  double* nm_part = nullptr;       // device scratch of rb_state_moments: the chunk partials, grown on demand
  size_t nm_cap = 0;               // its doubles
};

// Reader protocol (Ring::read_stream): ring_begin_read before enqueuing reads on s (orders them
// after the writes and the earlier readers of other streams), ring_end_read after them.
int ring_begin_read(Ring* r, hipStream_t s);
int ring_end_read(Ring* r, hipStream_t s);
// Writer protocol (Ring::write_stream): ring_begin_write before enqueuing writes of the records or d_size
// on s (orders them after every read and every other-stream write queued so far), ring_end_write after.
int ring_begin_write(Ring* r, hipStream_t s);
int ring_end_write(Ring* r, hipStream_t s);
// A stream that is about to be destroyed (synchronised by the caller) stops being a ring's
// noted reader / writer.
void ring_forget_stream(hipStream_t s);
// True while `r` is a live ring of allocation generation `gen` (not destroyed, not reused).
bool ring_alive(const Ring* r, uint64_t gen);

// One gather destination: rows [0, Bp) of dst[r*ld + col + c] = record[src + c], c < len.
struct GatherSeg {
  float* dst;
  int ld, col, src, len;
};

constexpr int kMaxSegs = 12;
constexpr int kMaxRecord = 2048;   // records up to this width are staged whole in LDS; wider
                                   // records (particle rings) are gathered segment by segment
struct GatherArgs {
  GatherSeg seg[kMaxSegs];
  int nseg;
  int B, Bp;
  const float* data;
  int rec;
  const int64_t* d_size;        // sample range [0, *d_size)
  const int64_t* inject_idx;    // nullable: use these rows instead of Philox
  int64_t* idx_out;             // nullable: record drawn rows
  uint64_t seed;
  const Counters* ctr;          // nullable: Philox step = ctr->total_it + 1
  uint64_t step;                // used when ctr == nullptr
};

int launch_gather(const GatherArgs& a, hipStream_t s);

// The mixed input launch (mixed.hip; include/td3.h "Demonstration replay"): batch rows [0, n_demo)
// from side 0, rows [n_demo, B) from side 1, each drawn as gather_row_index draws it on its own ring
// (the batch row is the Philox counter on both sides), rows [B, Bp) zero.  Both rings share the
// record layout (rec and the segments' src columns).  pbatch (particle learners, else null): the
// record's two particle blocks [o_p, o_p + np) and [o_p2, o_p2 + np) go to pbatch[row][2 np] as s | s'.
constexpr int kMixedSegs = kMaxSegs + 2;   // a staged particle record's blocks travel as two more segments
struct MixedSide {
  const float* data;
  const int64_t* d_size;
  uint64_t seed;
};
struct MixedArgs {
  GatherSeg seg[kMixedSegs];
  int nseg;
  int B, Bp, n_demo;
  int rec;
  MixedSide side[2];
  const int64_t* inject_idx;    // nullable: [B], the first n_demo rows of side 0, the rest of side 1
  int64_t* idx_out;             // nullable
  const Counters* ctr;          // Philox step = ctr->total_it + 1
  float* pbatch;
  int np, o_p, o_p2;
};
int launch_mixed_gather(const MixedArgs& a, hipStream_t s);

// The prioritized draw of `batch` rows on `s` (rb_sample_prioritized, include/td3.h): the rows into
// idx_out and idx_out2 (nullable), the importance weights, normalised by the batch maximum, into
// weight_out.  inject_u: device, nullable.  The caller holds the ring's read section and has checked
// that priorities are on and the ring is not empty.
int ring_draw_prioritized(Ring* r, int batch, double beta, const float* inject_u, int64_t* idx_out,
                          int64_t* idx_out2, float* weight_out, hipStream_t s);
// Leaves idx[0..n) = p (td = false) or (p + eps)^alpha (td = true), max_priority raised, parents
// repaired, on `s` (device arrays).  No stream ordering of its own: the caller's section provides it.
int ring_store_priorities(Ring* r, const int64_t* idx, const float* p, int64_t n, bool td, hipStream_t s);

// The ring-side members of a gather from `r` (the caller adds the segments, the batch and the draw).
inline GatherArgs gather_base(const Ring* r) {
  GatherArgs a{};
  a.data = r->data;
  a.rec = r->rec;
  a.d_size = r->d_size;
  a.seed = r->seed;
  return a;
}

}  // namespace td3
