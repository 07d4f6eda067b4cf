// link_amd/csrc/track.hip -- the CenterPoint tracker on the device (section Q of include/link_amd.h): greedy centre matching of one
// frame's detections against the track list, for a batch of independent sequences, one launch, no host read-back.
//
// Semantics, line by line: detection/tools/nusc_tracking/pub_tracker.py:45-154 (PubTracker.reset, step_centertrack) with
// detection/tools/nusc_tracking/track_utils.py:3-12 (greedy_assignment), and detection/tools/waymo_tracking/tracker.py:42-136 (the
// same algorithm with `score > score_thresh` on new tracks, :113).  The quirks are kept: the matched position is
// float32(ct + float32(tracking)) (pub_tracker.py:71-74), the distance is fp32 and compared strictly (`dist > max_diff`, :92), the
// first minimum wins (argmin, track_utils.py:8), a carried-over track moves by its OWN old `tracking`, whatever the present time
// lag is (:147-150), and it comes back with active = 0 + 1 (:127).  One deliberate difference: a frame whose detections are all of
// untracked classes clears the track list like an empty frame (:50-52); the reference raises an IndexError there (results[0], :71).
// The implementation is this project's.
//
// Contraction is off: the pose transform and the distance are sums of products that the reference rounds one by one.
#pragma clang fp contract(off)
#include <math.h>

#include "block_prims.h"

using namespace link;

namespace {

constexpr int TB = 512;                        // one workgroup per sequence: eight waves take the tracking classes in turn
constexpr int NW = TB / WAVE;
constexpr int HDR_BYTES = 32;                  // int32 n_tracks, id_count, status, capacity, 4 x reserved

// One list of `cap` tracks inside the state of a sequence: ct f64[cap][2], tracking f64[cap][2], then five int32[cap].
struct TrackList {
  double *ct, *tr;
  int32_t *label, *id, *age, *active, *src;
};
constexpr size_t list_bytes(int cap) { return (size_t)cap * (16 + 16 + 5 * 4); }
__device__ __forceinline__ TrackList list_at(unsigned char *p, int cap) {
  TrackList l;
  l.ct = reinterpret_cast<double *>(p);
  l.tr = l.ct + 2 * (size_t)cap;
  l.label = reinterpret_cast<int32_t *>(l.tr + 2 * (size_t)cap);
  l.id = l.label + cap;
  l.age = l.id + cap;
  l.active = l.age + cap;
  l.src = l.active + cap;
  return l;
}

struct TrackArgs {
  const float *boxes, *scores;
  const void *labels;
  const int32_t *counts;
  const double *time_lag;
  const uint8_t *reset;
  const double *pose;
  unsigned char *state;
  int32_t *det_id, *det_active;
  size_t state_stride;
  int32_t n, c, labels64;
  link_track_cfg_t cfg;
};

// minimum of a 64-bit key over the wave, in every lane: four DPP steps inside each row of 16 lanes (lane ^ 1, lane ^ 2, the mirror of
// the half row, the mirror of the row), then the four rows' results through readlane.  A lane whose DPP source is switched off keeps
// its own value (old = the value itself), so the step is a minimum with itself there.
template <int CTRL>
__device__ __forceinline__ uint64_t dpp_min_step(uint64_t v) {
  const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
  const uint32_t olo = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
  const uint32_t ohi = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false);
  const uint64_t o = ((uint64_t)ohi << 32) | olo;
  return o < v ? o : v;
}
__device__ __forceinline__ uint64_t wave_min_key(uint64_t v) {
  v = dpp_min_step<0xB1>(v);                   // quad_perm [1, 0, 3, 2]
  v = dpp_min_step<0x4E>(v);                   // quad_perm [2, 3, 0, 1]
  v = dpp_min_step<0x141>(v);                  // row_half_mirror
  v = dpp_min_step<0x140>(v);                  // row_mirror
  uint64_t best = ~0ull;
#pragma unroll
  for (int row = 0; row < 4; ++row) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 16 * row);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 16 * row);
    const uint64_t r = ((uint64_t)hi << 32) | lo;
    best = r < best ? r : best;
  }
  return best;
}

// centre and `tracking` of the detection in `slot`, in float64 (steps 4 and 5 of the header's list)
__device__ __forceinline__ void det_geom(const float *b, int c, const double *P, double lag, double ct[2], double tr[2]) {
  const double x = (double)b[0], y = (double)b[1], z = (double)b[2];
  double vx = (double)b[c - 3], vy = (double)b[c - 2];
  if (P) {
    ct[0] = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
    ct[1] = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
    const double gx = P[0] * vx + P[1] * vy, gy = P[4] * vx + P[5] * vy;
    vx = gx;
    vy = gy;
  } else {
    ct[0] = x;
    ct[1] = y;
  }
  tr[0] = (vx * -1.0) * lag;
  tr[1] = (vy * -1.0) * lag;
}

// LDS (dynamic): int tlab[K], float cx[K], cy[K], int cj[K], tmatch[K]; float dx[N], dy[N]; int dlab[N], dslot[N], dmatch[N].
// cx / cy / cj hold the old tracks sorted by class (stable), class c at s_off[c] .. s_off[c + 1].
__global__ __launch_bounds__(TB) void k_track_step(const TrackArgs a) {
  extern __shared__ int32_t smem[];
  __shared__ int s_w[NW], s_cnt[LINK_TRACK_MAX_LABELS], s_off[LINK_TRACK_MAX_LABELS + 1], s_map[LINK_TRACK_MAX_LABELS];
  __shared__ float s_md[LINK_TRACK_MAX_LABELS];
  const int K = a.cfg.capacity, N = a.n, C = a.c, ntl = a.cfg.n_track_labels, ndl = a.cfg.n_det_labels;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int32_t *tlab = smem;
  float *cx = reinterpret_cast<float *>(tlab + K), *cy = cx + K;
  int32_t *cj = reinterpret_cast<int32_t *>(cy + K), *tmatch = cj + K;
  float *dx = reinterpret_cast<float *>(tmatch + K), *dy = dx + N;
  int32_t *dlab = reinterpret_cast<int32_t *>(dy + N), *dslot = dlab + N, *dmatch = dslot + N;

  unsigned char *st = a.state + (size_t)s * a.state_stride;
  int32_t *hdr = reinterpret_cast<int32_t *>(st);
  const TrackList cur = list_at(st + HDR_BYTES, K), nxt = list_at(st + HDR_BYTES + list_bytes(K), K);
  const bool rst = a.reset && a.reset[s];
  int M = rst ? 0 : hdr[0];
  M = M < 0 ? 0 : (M > K ? K : M);
  const int idc = rst ? 0 : hdr[1];
  const double lag = a.time_lag[s];
  const double *P = a.pose ? a.pose + 12 * (size_t)s : nullptr;
  int cnt = N;
  if (a.counts) {
    cnt = a.counts[s];
    cnt = cnt < 0 ? 0 : (cnt > N ? N : cnt);
  }
  const float *boxes = a.boxes + (size_t)s * N * C;
  const float *scores = a.scores + (size_t)s * N;
  int32_t *det_id = a.det_id + (size_t)s * N, *det_active = a.det_active + (size_t)s * N;

  if (tid < LINK_TRACK_MAX_LABELS) {
    s_cnt[tid] = 0;
    s_map[tid] = a.cfg.label_map[tid];
    s_md[tid] = a.cfg.max_dist[tid];
  }
  __syncthreads();

  // 1. the detections of tracked classes, packed in order (step 3), with their matched position in fp32 (step 6)
  int nd = 0;
  for (int base = 0; base < N; base += TB) {
    const int i = base + tid;
    int tl = -1;
    if (i < N) {
      det_id[i] = -1;
      det_active[i] = 0;
      if (i < cnt) {
        const int64_t lab = a.labels64 ? reinterpret_cast<const int64_t *>(a.labels)[(size_t)s * N + i]
                                       : (int64_t) reinterpret_cast<const int32_t *>(a.labels)[(size_t)s * N + i];
        if (lab >= 0 && lab < ndl) tl = s_map[lab];
      }
    }
    int tot;
    const int r = block_rank<TB>(tl >= 0, s_w, tot);
    if (tl >= 0) {
      const int q = nd + r;
      double ct[2], tr[2];
      det_geom(boxes + (size_t)i * C, C, P, lag, ct, tr);
      dx[q] = (float)(ct[0] + (double)(float)tr[0]);
      dy[q] = (float)(ct[1] + (double)(float)tr[1]);
      dlab[q] = tl;
      dslot[q] = i;
      dmatch[q] = -1;
    }
    nd += tot;
  }
  if (nd == 0) M = 0;                          // step 2: nothing to match clears the list (id_count stays)

  // 2. the old tracks: class histogram, then a stable sort by class into cx / cy / cj
  for (int j = tid; j < M; j += TB) {
    const int l = cur.label[j];
    tlab[j] = l;
    tmatch[j] = -1;
    if ((unsigned)l < (unsigned)ntl) atomicAdd(&s_cnt[l], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int c = 0; c < ntl; ++c) {
      s_off[c] = acc;
      acc += s_cnt[c];
    }
    s_off[ntl] = acc;
  }
  __syncthreads();

  // 3. one greedy scan per class, the waves taking the classes in turn.  A detection can only match a track of its class and a
  // taken track only matters to that class, so the N-long scan of the reference splits into these without changing any decision.
  // No workgroup barrier inside: a wave packs its class's tracks, a lane owns tracks k = lane, lane + 64, .. of the class with a
  // `taken` bit each in a register, and a detection costs one pass over the lane's share and one wave minimum on
  // (distance bits, k), which is the first minimum in track order.
  for (int c = w; c < ntl; c += NW) {
    const int off = s_off[c], mc = s_off[c + 1] - off;
    if (mc == 0) continue;
    int k0 = 0;
    for (int base = 0; base < M; base += WAVE) {
      const int j = base + lane;
      const bool p = j < M && tlab[j] == c;
      const uint64_t m = __ballot(p);
      if (p) {
        const int q = off + k0 + __popcll(m & ((1ull << lane) - 1ull));
        cx[q] = (float)cur.ct[2 * j];          // step 7
        cy[q] = (float)cur.ct[2 * j + 1];
        cj[q] = j;
      }
      k0 += __popcll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const float md = s_md[c];
    uint32_t taken = 0;                        // bit t: track k = lane + 64 t of this class is taken (mc <= 1024: 16 bits)
    for (int base = 0; base < nd; base += WAVE) {
      const int i = base + lane;
      uint64_t m = __ballot(i < nd && dlab[i] == c);
      while (m) {
        const int d = base + (int)__ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const float px = dx[d], py = dy[d];
        uint64_t best = ~0ull;
        int t = 0;
        for (int k = lane; k < mc; k += WAVE, ++t) {
          if ((taken >> t) & 1u) continue;
          const float ex = cx[off + k] - px, ey = cy[off + k] - py;
          const float s2 = ex * ex + ey * ey;
          const float dist = (float)sqrt((double)s2);      // fp64 root rounded to fp32: the correctly rounded fp32 root (53 >= 2 * 24 + 2)
          if (!(dist > md) && dist < 1e16f) {              // step 9; track_utils.py:9
            const uint64_t key = ((uint64_t)__float_as_uint(dist) << 32) | (uint32_t)k;
            best = key < best ? key : best;
          }
        }
        best = wave_min_key(best);
        if (best != ~0ull) {
          const int kb = (int)(uint32_t)best;
          if (lane == (kb & 63)) taken |= 1u << (kb >> 6);
          if (lane == 0) {
            const int j = cj[off + kb];
            dmatch[d] = j;
            tmatch[j] = d;
          }
        }
      }
    }
  }
  __syncthreads();

  // 4. the new list: matched detections, new tracks, carried-over tracks (step 11), written into the second list
  int nm = 0, nn = 0;
  const float th = a.cfg.score_thresh;
  const bool no_th = th != th;
  for (int base = 0; base < nd; base += TB) {
    const int q = base + tid;
    const bool valid = q < nd;
    const int j = valid ? dmatch[q] : -1;
    const bool ism = valid && j >= 0;
    const bool isn = valid && j < 0 && (no_th || scores[dslot[q]] > th);
    int tm, tn;
    block_rank<TB>(ism, s_w, tm);
    block_rank<TB>(isn, s_w, tn);
    nm += tm;
    nn += tn;
  }
  int bm = 0, bn = 0;
  for (int base = 0; base < nd; base += TB) {
    const int q = base + tid;
    const bool valid = q < nd;
    const int j = valid ? dmatch[q] : -1;
    const int slot = valid ? dslot[q] : 0;
    const bool ism = valid && j >= 0;
    const bool isn = valid && j < 0 && (no_th || scores[slot] > th);
    int tm, tn;
    const int rm = block_rank<TB>(ism, s_w, tm);
    const int rn = block_rank<TB>(isn, s_w, tn);
    if (ism || isn) {
      const int pos = ism ? bm + rm : nm + bn + rn;      // < nd <= N <= K
      double ct[2], tr[2];
      det_geom(boxes + (size_t)slot * C, C, P, lag, ct, tr);
      const int id = ism ? cur.id[j] : idc + bn + rn + 1;
      const int act = ism ? cur.active[j] + 1 : 1;
      nxt.ct[2 * pos] = ct[0];
      nxt.ct[2 * pos + 1] = ct[1];
      nxt.tr[2 * pos] = tr[0];
      nxt.tr[2 * pos + 1] = tr[1];
      nxt.label[pos] = dlab[q];
      nxt.id[pos] = id;
      nxt.age[pos] = 1;
      nxt.active[pos] = act;
      nxt.src[pos] = slot;
      det_id[slot] = id;
      det_active[slot] = act;
    }
    bm += tm;
    bn += tn;
  }
  int bc = 0;
  for (int base = 0; base < M; base += TB) {
    const int j = base + tid;
    const bool car = j < M && tmatch[j] < 0 && cur.age[j] < a.cfg.max_age;
    int tc;
    const int rc = block_rank<TB>(car, s_w, tc);
    const int pos = nm + nn + bc + rc;
    if (car && pos < K) {
      nxt.ct[2 * pos] = cur.ct[2 * j] - cur.tr[2 * j];
      nxt.ct[2 * pos + 1] = cur.ct[2 * j + 1] - cur.tr[2 * j + 1];
      nxt.tr[2 * pos] = cur.tr[2 * j];
      nxt.tr[2 * pos + 1] = cur.tr[2 * j + 1];
      nxt.label[pos] = tlab[j];
      nxt.id[pos] = cur.id[j];
      nxt.age[pos] = cur.age[j] + 1;
      nxt.active[pos] = 0;
      nxt.src[pos] = -1;
    }
    bc += tc;
  }
  const int total = nm + nn + bc, kept = total > K ? K : total;
  __threadfence_block();
  __syncthreads();

  // 5. the second list becomes the first: every read of the old list is behind the barrier above
  for (int i = tid; i < kept; i += TB) {
    cur.ct[2 * i] = nxt.ct[2 * i];
    cur.ct[2 * i + 1] = nxt.ct[2 * i + 1];
    cur.tr[2 * i] = nxt.tr[2 * i];
    cur.tr[2 * i + 1] = nxt.tr[2 * i + 1];
    cur.label[i] = nxt.label[i];
    cur.id[i] = nxt.id[i];
    cur.age[i] = nxt.age[i];
    cur.active[i] = nxt.active[i];
    cur.src[i] = nxt.src[i];
  }
  if (tid == 0) {
    hdr[0] = kept;
    hdr[1] = idc + nn;
    hdr[2] = total > K ? LINK_TRACK_STATUS_OVERFLOW : 0;
    hdr[3] = K;
  }
}

}  // namespace

extern "C" size_t link_track_state_bytes(int32_t capacity) {
  if (capacity < 1 || capacity > LINK_TRACK_MAX_CAPACITY) return 0;
  return HDR_BYTES + 2 * list_bytes(capacity);
}

extern "C" int link_track_step(const link_track_cfg_t *cfg, int32_t n_seq, int32_t n, int32_t box_len, const float *boxes,
                               const float *scores, const void *labels, int32_t labels_int64, const int32_t *counts,
                               const double *time_lag, const uint8_t *reset, const double *pose, void *state, int32_t *det_tracking_id,
                               int32_t *det_active, void *stream) {
  if (!cfg || n_seq < 0 || n < 0) return LINK_ERR_ARG;
  if (cfg->capacity < 1 || cfg->capacity > LINK_TRACK_MAX_CAPACITY || n > cfg->capacity || cfg->max_age < 0) return LINK_ERR_ARG;
  if (cfg->n_det_labels < 1 || cfg->n_det_labels > LINK_TRACK_MAX_LABELS || cfg->n_track_labels < 1 ||
      cfg->n_track_labels > LINK_TRACK_MAX_LABELS)
    return LINK_ERR_ARG;
  for (int i = 0; i < cfg->n_det_labels; ++i)
    if (cfg->label_map[i] < -1 || cfg->label_map[i] >= cfg->n_track_labels) return LINK_ERR_ARG;
  for (int i = 0; i < cfg->n_track_labels; ++i)
    if (!(cfg->max_dist[i] >= 0.0f && cfg->max_dist[i] < 1e16f)) return LINK_ERR_ARG;
  if (n_seq == 0) return LINK_OK;
  if (!time_lag || !state) return LINK_ERR_ARG;
  if (n > 0 && (box_len < 6 || box_len > 64 || !boxes || !scores || !labels || !det_tracking_id || !det_active)) return LINK_ERR_ARG;
  TrackArgs a;
  a.boxes = boxes; a.scores = scores; a.labels = labels; a.counts = counts; a.time_lag = time_lag; a.reset = reset; a.pose = pose;
  a.state = static_cast<unsigned char *>(state); a.det_id = det_tracking_id; a.det_active = det_active;
  a.state_stride = link_track_state_bytes(cfg->capacity);
  a.n = n; a.c = box_len; a.labels64 = labels_int64 ? 1 : 0;
  a.cfg = *cfg;
  const size_t lds = ((size_t)cfg->capacity + (size_t)n) * 5 * sizeof(int32_t);      // <= 40 KiB
  hipLaunchKernelGGL(k_track_step, dim3((unsigned)n_seq), dim3(TB), lds, S(stream), a);
  return check_launch("link_track_step");
}
