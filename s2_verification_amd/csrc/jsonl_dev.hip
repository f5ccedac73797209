// jsonl_dev.hip — collector JSONL decoded on the GPU into binary cache
// sections (cache.cpp's mode 0), SURVEY.md §8f row 3's device half.
//
// Per chunk of staged text (every history's records each end with one '\n';
// the host appends the final one where a history lacks it):
//   jd_count_nl / jd_scan_u32 / jd_scatter_nl   newline positions = record ends
//   jd_hist_ranges   each history's record range (binary search of its bounds)
//   jd_parse         one lane per record: jd::parse_record
//   jd_hist          one wave per history, a tile of records at a time: all
//                    lanes scan the hash offsets and stage what the pass
//                    reads in LDS, then lane 0 makes jd::seq_step's pass (ids,
//                    colouring, interning); at the end the section's size
//   jd_scan_sizes    exclusive scan of the section sizes (on the device)
//   jd_layout        one block per history writes its section
// A history the device refuses (any deviating byte, a structural case, a cap)
// has section size 0 and takes load_jsonl_finalized on the host.
//
// Bounds: every text read is inside a record [start, end) with end a newline
// position < the staged length, or a 16-byte tile below the staged length plus
// its zero pad; every array write is guarded by the array's capacity (records
// by rec_cap, sections by out_cap), so no input can move an access outside a
// buffer.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "history.h"
#include "host_par.h"
#include "jsonl_dev.h"
#include "s2lincheck.h"
#include "search.h"

namespace s2lc {

static_assert(H_NOWRAP == 0x1 && H_P2OK == 0x2 && H_P4 == 0x4 && H_IDEFER == 0x8 && H_TAIL32 == 0x10,
              "jd::seq_finish writes these bits");
static_assert(offsetof(OpRec, sufmin) == 32 && offsetof(OpRec, call_ev) == 40 && offsetof(OpRec, ret_ev) == 44 &&
                  offsetof(OpRec, hash_off) == 48 && offsetof(OpRec, hash_cnt) == 52 && offsetof(OpRec, batch_tok) == 56 &&
                  offsetof(OpRec, set_tok) == 58 && offsetof(OpRec, flags) == 60,
              "jd::layout_fill writes an OpRec as eight words");

namespace {

using jd::MAX_CHAINS;
using jd::MAX_TOKENS;

constexpr uint32_t TILE = 4096;       // text bytes per block of jd_count_nl / jd_scatter_nl (256 lanes x 16)
constexpr uint32_t CS_STRIDE = MAX_CHAINS + 1;
constexpr uint32_t MAX_CHUNK_HIST = 16384;

using JdHist = jd::Hist;

// exclusive scan of v over a 256- or 1024-lane block; *total = the block's sum
template <typename T>
__device__ T block_scan(T v, T* total, T* sm) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  T inc = v;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const T t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  if (lane == 63) sm[w] = inc;
  __syncthreads();
  T base = 0, tot = 0;
  for (uint32_t k = 0; k < nw; ++k) {
    if (k < w) base += sm[k];
    tot += sm[k];
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

__device__ inline uint32_t nl_in_word(uint32_t w) {
  uint32_t c = 0;
  for (int k = 0; k < 4; ++k) c += ((w >> (8 * k)) & 0xFF) == '\n';
  return c;
}

// newlines of tile blockIdx.x (text_len rounded up to 16 is inside the padded buffer)
__global__ __launch_bounds__(256) void jd_count_nl(const uint8_t* __restrict__ text, uint32_t text_len,
                                                   uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t sm[16];
  const uint64_t off = (uint64_t)blockIdx.x * TILE + threadIdx.x * 16;
  uint32_t c = 0;
  if (off < text_len) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + off);
    c = nl_in_word(v.x) + nl_in_word(v.y) + nl_in_word(v.z) + nl_in_word(v.w);
  }
  uint32_t tot;
  block_scan<uint32_t>(c, &tot, sm);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = tot;
}

// in-place exclusive scan of a[0, n) by one block; *total = the sum
__global__ __launch_bounds__(1024) void jd_scan_u32(uint32_t* __restrict__ a, uint32_t n, uint32_t* __restrict__ total) {
  __shared__ uint32_t sm[16];
  uint32_t carry = 0;
  for (uint32_t b = 0; b < n; b += blockDim.x) {
    const uint32_t i = b + threadIdx.x;
    const uint32_t v = i < n ? a[i] : 0;
    uint32_t tot;
    const uint32_t ex = block_scan<uint32_t>(v, &tot, sm);
    if (i < n) a[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void jd_scatter_nl(const uint8_t* __restrict__ text, uint32_t text_len,
                                                     const uint32_t* __restrict__ tile_off,
                                                     uint32_t* __restrict__ nl_pos, uint32_t rec_cap) {
  __shared__ uint32_t sm[16];
  const uint64_t off = (uint64_t)blockIdx.x * TILE + threadIdx.x * 16;
  uint32_t w[4] = {0, 0, 0, 0};
  uint32_t c = 0;
  if (off < text_len) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + off);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    c = nl_in_word(w[0]) + nl_in_word(w[1]) + nl_in_word(w[2]) + nl_in_word(w[3]);
  }
  uint32_t tot;
  uint32_t idx = tile_off[blockIdx.x] + block_scan<uint32_t>(c, &tot, sm);
  if (!c) return;
  for (int k = 0; k < 16; ++k) {
    if (((w[k >> 2] >> (8 * (k & 3))) & 0xFF) != '\n') continue;
    if (idx < rec_cap) nl_pos[idx] = (uint32_t)off + k;
    ++idx;
  }
}

// first index in nl_pos[0, n) with nl_pos[i] >= x
__device__ inline uint32_t lower_bound(const uint32_t* __restrict__ nl_pos, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (nl_pos[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ void jd_hist_ranges(const uint32_t* __restrict__ h_off, uint32_t nh, const uint32_t* __restrict__ nl_pos,
                               const uint32_t* __restrict__ n_nl, uint32_t rec_cap, JdHist* __restrict__ hist) {
  const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= nh) return;
  const uint32_t nr = min(*n_nl, rec_cap);
  const uint32_t a = h_off[h], b = h_off[h + 1];
  JdHist o{};
  if (b > a) {
    const uint32_t lo = lower_bound(nl_pos, nr, a), hi = lower_bound(nl_pos, nr, b);
    o.rec_base = lo;
    o.n_rec = hi - lo;
    // its last byte is a newline (the host staged it so): present unless the record cap cut the list
    o.ok = hi > lo && nl_pos[hi - 1] == b - 1;
  } else {
    o.ok = 1;  // an empty history: no records
  }
  hist[h] = o;
}

__global__ __launch_bounds__(256) void jd_parse(const uint8_t* __restrict__ text, const uint32_t* __restrict__ nl_pos,
                                                const uint32_t* __restrict__ n_nl, uint32_t rec_cap,
                                                jd::Rec* __restrict__ recs) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= min(*n_nl, rec_cap)) return;
  const uint32_t start = r ? nl_pos[r - 1] + 1 : 0, end = nl_pos[r];
  jd::Rec e;
  jd::parse_record(text, start, end, e);
  recs[r] = e;
}

// one wave per history
constexpr uint32_t SEQ_TILE = 256;  // records staged in LDS per step of the sequential pass

__global__ __launch_bounds__(64) void jd_hist(const uint8_t* __restrict__ text, const jd::Rec* __restrict__ recs,
                                              JdHist* __restrict__ hist, jd::Op* __restrict__ ops,
                                              uint32_t* __restrict__ tokid, uint32_t* __restrict__ hash_off,
                                              uint32_t* __restrict__ chains, jd::TokRef* __restrict__ toks) {
  __shared__ uint32_t last[MAX_CHAINS], chain_len[MAX_CHAINS], open_op[MAX_CHAINS], tlen[MAX_TOKENS];
  __shared__ uint64_t tkey[MAX_TOKENS];
  __shared__ jd::SeqIn tile[SEQ_TILE];
  __shared__ uint32_t refused;
  const uint32_t h = blockIdx.x, lane = threadIdx.x;
  JdHist hi = hist[h];
  if (!hi.ok) return;
  const uint32_t base = hi.rec_base, n = hi.n_rec;
  jd::TokRef* tk = toks + (size_t)h * MAX_TOKENS;
  jd::Seq S;  // (lane 0's)
  S.text = text;
  S.ops = ops + base;
  S.tokid = tokid + base;
  S.toks = tk;
  S.last = last;
  S.chain_len = chain_len;
  S.open_op = open_op;
  S.tkey = tkey;
  S.tlen = tlen;
  if (lane == 0) refused = 0;
  __syncthreads();
  uint32_t carry = 0;  // exclusive scan of hash_cnt over the history's records
  for (uint32_t t0 = 0; t0 < n; t0 += SEQ_TILE) {
    const uint32_t tn = min(SEQ_TILE, n - t0);
    for (uint32_t b = 0; b < tn; b += 64) {
      const uint32_t i = b + lane;
      uint32_t v = 0;
      if (i < tn) {
        const jd::Rec& r = recs[base + t0 + i];
        v = r.hash_cnt;
        tile[i] = jd::seq_in(text, r);
      }
      uint32_t inc = v;
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
      }
      if (i < tn) hash_off[base + t0 + i] = carry + inc - v;
      carry += __shfl(inc, 63, 64);
    }
    __syncthreads();
    if (lane == 0) {
      for (uint32_t i = 0; i < tn; ++i)
        if (!jd::seq_step(S, t0 + i, tile[i])) {
          refused = 1;
          break;
        }
    }
    __syncthreads();
    if (refused) break;
  }
  if (lane != 0) return;
  jd::HistOut out{};
  if (!refused && jd::seq_finish(S, out)) {
    jd::finish_hist(hi, out, carry, chain_len, tk, chains + (size_t)h * CS_STRIDE);
  } else {
    hi.ok = 0;
    hi.sec_size = 0;
  }
  hist[h] = hi;
}

// sec_off[0, nh] = exclusive scan of the section sizes, by one block
__global__ __launch_bounds__(1024) void jd_scan_sizes(const JdHist* __restrict__ hist, uint32_t nh,
                                                      uint64_t* __restrict__ sec_off) {
  __shared__ uint64_t sm[16];
  uint64_t carry = 0;
  for (uint32_t b = 0; b < nh; b += blockDim.x) {
    const uint32_t i = b + threadIdx.x;
    const uint64_t v = i < nh ? hist[i].sec_size : 0;
    uint64_t tot;
    const uint64_t ex = block_scan<uint64_t>(v, &tot, sm);
    if (i < nh) sec_off[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) sec_off[nh] = carry;
}

// one block per history: its section, as write_section (cache.cpp) lays it out
__global__ __launch_bounds__(256) void jd_layout(const uint8_t* __restrict__ text, const jd::Rec* __restrict__ recs,
                                                 const JdHist* __restrict__ hist, const jd::Op* __restrict__ ops,
                                                 const uint32_t* __restrict__ tokid,
                                                 const uint32_t* __restrict__ hash_off,
                                                 const uint32_t* __restrict__ chains,
                                                 const jd::TokRef* __restrict__ toks,
                                                 const uint64_t* __restrict__ sec_off, uint8_t* __restrict__ out,
                                                 uint64_t out_cap) {
  const uint32_t h = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const JdHist hi = hist[h];
  if (!hi.ok) return;
  const uint64_t off = sec_off[h];
  if (off + hi.sec_size > out_cap) return;  // (the host sends this history to the CPU decoder)
  const uint32_t base = hi.rec_base;
  const jd::Layout L{text, recs + base, ops + base, tokid + base, hash_off + base, chains + (size_t)h * CS_STRIDE,
                     toks + (size_t)h * MAX_TOKENS, out + off};
  __shared__ uint32_t n_ident;
  if (tid == 0) n_ident = 0;
  __syncthreads();
  const uint32_t mine = jd::layout_fill(L, hi, tid, nt);
  if (mine) atomicAdd(&n_ident, mine);
  __syncthreads();  // (the block's fills are visible to its lanes: sufmin reads other lanes' records)
  if (tid == 0) jd::layout_head(L, hi, n_ident);
  jd::layout_sufmin(L, hi, tid, nt);
}

#define JDCHK(x)                                                                                  \
  do {                                                                                            \
    hipError_t e_ = (x);                                                                          \
    if (e_ != hipSuccess) {                                                                       \
      err = std::string("device decode: " #x ": ") + hipGetErrorString(e_);                       \
      return S2LC_EHIP;                                                                           \
    }                                                                                             \
  } while (0)

struct Buf {  // grow-only
  void* p = nullptr;
  size_t cap = 0;
  bool pinned = false;
  hipError_t need(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    const size_t want = n + n / 4;
    const hipError_t e = pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
    if (e != hipSuccess) { p = nullptr; return e; }
    cap = want;
    return hipSuccess;
  }
  void release() {
    if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

struct Slot {
  hipStream_t stream = nullptr;
  hipEvent_t ev[6] = {};  // h2d start/end, kernels end, meta copied, d2h start/end
  Buf h_text, h_hoff, h_hist, h_secoff, h_out;
  Buf d_text, d_hoff, d_tile, d_nl, d_recs, d_hashoff, d_tokid, d_ops, d_hist, d_chains, d_toks, d_secoff, d_out, d_nnl;
  // the chunk in flight
  size_t first = 0, nh = 0;
  uint64_t text_len = 0, out_cap = 0;
  Slot() { h_text.pinned = h_hoff.pinned = h_hist.pinned = h_secoff.pinned = h_out.pinned = true; }
  Buf* all[19] = {&h_text, &h_hoff, &h_hist, &h_secoff, &h_out, &d_text, &d_hoff, &d_tile, &d_nl, &d_recs,
                  &d_hashoff, &d_tokid, &d_ops, &d_hist, &d_chains, &d_toks, &d_secoff, &d_out, &d_nnl};
};

}  // namespace

struct JdState {
  Slot slot[2];
  bool ready = false;
};

void jd_release(JdState* s) {
  if (!s) return;
  for (Slot& sl : s->slot) {
    for (Buf* b : sl.all) b->release();
    for (hipEvent_t e : sl.ev)
      if (e) (void)hipEventDestroy(e);
    if (sl.stream) (void)hipStreamDestroy(sl.stream);
  }
  delete s;
}

namespace {

size_t chunk_bytes() {
  size_t mb = 512;
  if (const char* e = getenv("S2LC_DEVDECODE_CHUNK_MB")) {
    const long v = strtol(e, nullptr, 10);
    if (v >= 1) mb = (size_t)std::min<long>(v, 2048);
  }
  return mb << 20;
}

// Stage chunk [first, first + nh) into the slot and enqueue its copy and kernels.
int launch_chunk(Slot& s, const uint8_t* const* bufs, const size_t* lens, size_t first, size_t nh, JdStats& st,
                 std::string& err) {
  const int64_t t0 = steady_ns();
  s.first = first;
  s.nh = nh;
  JDCHK(s.h_hoff.need((nh + 1) * 4));
  uint32_t* hoff = s.h_hoff.as<uint32_t>();
  uint64_t pos = 0;
  for (size_t i = 0; i < nh; ++i) {
    hoff[i] = (uint32_t)pos;
    const size_t len = lens[first + i];
    pos += len + ((len && bufs[first + i][len - 1] != '\n') ? 1 : 0);
  }
  hoff[nh] = (uint32_t)pos;
  const uint64_t B = pos;  // (< 2^32: the caller bounds a chunk)
  s.text_len = B;
  JDCHK(s.h_text.need(B + jd::TEXT_PAD));
  uint8_t* ht = s.h_text.as<uint8_t>();
  parallel_for(nh, 8, [&](size_t i) {
    const size_t len = lens[first + i];
    if (!len) return;
    memcpy(ht + hoff[i], bufs[first + i], len);
    if (bufs[first + i][len - 1] != '\n') ht[hoff[i] + len] = '\n';
  });
  memset(ht + B, 0, jd::TEXT_PAD);
  st.stage_ms += 1e-6 * (steady_ns() - t0);
  st.bytes_in += B;

  // a record of the collector's form is at least 49 bytes and its newline
  const uint64_t rec_cap = B / 48 + nh + 16;
  const uint32_t ntiles = (uint32_t)((B + TILE - 1) / TILE);
  s.out_cap = 2 * B + 512ull * nh + 64;
  JDCHK(s.d_text.need(B + jd::TEXT_PAD));
  JDCHK(s.d_hoff.need((nh + 1) * 4));
  JDCHK(s.d_tile.need(((size_t)ntiles + 1) * 4));
  JDCHK(s.d_nnl.need(4));
  JDCHK(s.d_nl.need(rec_cap * 4));
  JDCHK(s.d_recs.need(rec_cap * sizeof(jd::Rec)));
  JDCHK(s.d_hashoff.need(rec_cap * 4));
  JDCHK(s.d_tokid.need(rec_cap * 4));
  JDCHK(s.d_ops.need(rec_cap * sizeof(jd::Op)));
  JDCHK(s.d_hist.need(nh * sizeof(JdHist)));
  JDCHK(s.d_chains.need(nh * CS_STRIDE * 4));
  JDCHK(s.d_toks.need(nh * MAX_TOKENS * sizeof(jd::TokRef)));
  JDCHK(s.d_secoff.need((nh + 1) * 8));
  JDCHK(s.d_out.need(s.out_cap));
  JDCHK(s.h_hist.need(nh * sizeof(JdHist)));
  JDCHK(s.h_secoff.need((nh + 1) * 8));

  hipStream_t q = s.stream;
  JDCHK(hipEventRecord(s.ev[0], q));
  JDCHK(hipMemcpyAsync(s.d_text.p, ht, B + jd::TEXT_PAD, hipMemcpyHostToDevice, q));
  JDCHK(hipMemcpyAsync(s.d_hoff.p, hoff, (nh + 1) * 4, hipMemcpyHostToDevice, q));
  JDCHK(hipEventRecord(s.ev[1], q));
  const uint8_t* text = s.d_text.as<uint8_t>();
  uint32_t* nnl = s.d_nnl.as<uint32_t>();
  if (ntiles) hipLaunchKernelGGL(jd_count_nl, dim3(ntiles), dim3(256), 0, q, text, (uint32_t)B, s.d_tile.as<uint32_t>());
  hipLaunchKernelGGL(jd_scan_u32, dim3(1), dim3(1024), 0, q, s.d_tile.as<uint32_t>(), ntiles, nnl);
  if (ntiles)
    hipLaunchKernelGGL(jd_scatter_nl, dim3(ntiles), dim3(256), 0, q, text, (uint32_t)B, s.d_tile.as<uint32_t>(),
                       s.d_nl.as<uint32_t>(), (uint32_t)rec_cap);
  hipLaunchKernelGGL(jd_hist_ranges, dim3((uint32_t)((nh + 255) / 256)), dim3(256), 0, q, s.d_hoff.as<uint32_t>(),
                     (uint32_t)nh, s.d_nl.as<uint32_t>(), nnl, (uint32_t)rec_cap, s.d_hist.as<JdHist>());
  hipLaunchKernelGGL(jd_parse, dim3((uint32_t)((rec_cap + 255) / 256)), dim3(256), 0, q, text, s.d_nl.as<uint32_t>(),
                     nnl, (uint32_t)rec_cap, s.d_recs.as<jd::Rec>());
  hipLaunchKernelGGL(jd_hist, dim3((uint32_t)nh), dim3(64), 0, q, text, s.d_recs.as<jd::Rec>(), s.d_hist.as<JdHist>(),
                     s.d_ops.as<jd::Op>(), s.d_tokid.as<uint32_t>(), s.d_hashoff.as<uint32_t>(),
                     s.d_chains.as<uint32_t>(), s.d_toks.as<jd::TokRef>());
  hipLaunchKernelGGL(jd_scan_sizes, dim3(1), dim3(1024), 0, q, s.d_hist.as<JdHist>(), (uint32_t)nh,
                     s.d_secoff.as<uint64_t>());
  hipLaunchKernelGGL(jd_layout, dim3((uint32_t)nh), dim3(256), 0, q, text, s.d_recs.as<jd::Rec>(),
                     s.d_hist.as<JdHist>(), s.d_ops.as<jd::Op>(), s.d_tokid.as<uint32_t>(),
                     s.d_hashoff.as<uint32_t>(), s.d_chains.as<uint32_t>(), s.d_toks.as<jd::TokRef>(),
                     s.d_secoff.as<uint64_t>(), s.d_out.as<uint8_t>(), s.out_cap);
  JDCHK(hipGetLastError());
  JDCHK(hipEventRecord(s.ev[2], q));
  JDCHK(hipMemcpyAsync(s.h_hist.p, s.d_hist.p, nh * sizeof(JdHist), hipMemcpyDeviceToHost, q));
  JDCHK(hipMemcpyAsync(s.h_secoff.p, s.d_secoff.p, (nh + 1) * 8, hipMemcpyDeviceToHost, q));
  JDCHK(hipEventRecord(s.ev[3], q));
  return 0;
}

// Wait for the slot's chunk, download its image and load the sections into
// pre[]; a history without a section goes on the fallback list.
int finish_chunk(Slot& s, s2lc_history** pre, uint8_t* on_device, std::vector<size_t>& fallback, JdStats& st,
                 std::string& err) {
  JDCHK(hipEventSynchronize(s.ev[3]));
  const JdHist* hist = s.h_hist.as<JdHist>();
  const uint64_t* so = s.h_secoff.as<uint64_t>();
  const size_t nh = s.nh;
  uint64_t image = 0;
  std::vector<uint8_t> have(nh, 0);
  for (size_t i = 0; i < nh; ++i) {
    if (!hist[i].ok || !hist[i].sec_size || so[i] + hist[i].sec_size > s.out_cap) continue;
    have[i] = 1;
    image = std::max(image, so[i] + hist[i].sec_size);
  }
  hipStream_t q = s.stream;
  JDCHK(s.h_out.need(image));
  JDCHK(hipEventRecord(s.ev[4], q));
  if (image) JDCHK(hipMemcpyAsync(s.h_out.p, s.d_out.p, image, hipMemcpyDeviceToHost, q));
  JDCHK(hipEventRecord(s.ev[5], q));
  JDCHK(hipEventSynchronize(s.ev[5]));
  float ms = 0;
  JDCHK(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
  st.h2d_ms += ms;
  JDCHK(hipEventElapsedTime(&ms, s.ev[1], s.ev[2]));
  st.kernel_ms += ms;
  JDCHK(hipEventElapsedTime(&ms, s.ev[4], s.ev[5]));
  st.d2h_ms += ms;
  st.bytes_out += image;
  const int64_t t0 = steady_ns();
  const uint8_t* img = s.h_out.as<uint8_t>();
  std::atomic<int> oom{0};
  parallel_for(nh, 8, [&](size_t i) {
    if (!have[i]) return;
    try {
      if (cache_section_load(img + so[i], img + so[i] + hist[i].sec_size, pre[s.first + i]->h)) {
        have[i] = 2;
      } else {
        pre[s.first + i]->h.recycle();
      }
    } catch (...) {
      oom = 1;
    }
  });
  if (oom) {
    err = "out of memory";
    return S2LC_ENOMEM;
  }
  for (size_t i = 0; i < nh; ++i) {
    if (have[i] == 2) {
      st.n_device++;
      if (on_device) on_device[s.first + i] = 1;
      continue;
    }
    if (have[i] == 1) st.n_rejected++;  // a section read_section refuses: a decoder bug
    fallback.push_back(s.first + i);
  }
  st.load_ms += 1e-6 * (steady_ns() - t0);
  return 0;
}

}  // namespace

// The histories bufs[0, n) into pre[0, n) (acquired by the caller): device
// sections where the device accepts, load_jsonl_finalized otherwise. rcs/errs
// [n] receive each fallback's status and message.
int jd_decode_many(JdState** state, int device, const uint8_t* const* bufs, const size_t* lens, size_t n,
                   int n_threads, s2lc_history** pre, uint8_t* on_device, JdStats& st, std::vector<int>& rcs,
                   std::vector<std::string>& errs, std::string& err) {
  JDCHK(hipSetDevice(device));
  if (!*state) *state = new JdState();
  JdState& S = **state;
  if (!S.ready) {
    for (Slot& s : S.slot)
      for (hipEvent_t& e : s.ev) JDCHK(hipEventCreate(&e));
    S.ready = true;
  }
  // The two streams live for this call only. A stream holds one of the
  // process's few hardware queues (4 by default) for as long as it exists, and
  // a context that kept two more would push the streams of every context
  // created after it onto shared queues.
  struct Streams {
    JdState& S;
    ~Streams() {
      for (Slot& s : S.slot) {
        if (!s.stream) continue;
        (void)hipStreamSynchronize(s.stream);  // nothing in flight reads a buffer we return
        (void)hipStreamDestroy(s.stream);
        s.stream = nullptr;
      }
    }
  } streams{S};
  for (Slot& s : S.slot) JDCHK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  std::vector<size_t> fallback;
  const size_t chunk = chunk_bytes();
  constexpr size_t kMaxDev = 0xF0000000ull;  // device offsets are 32-bit
  size_t i = 0;
  int k = 0;
  Slot* inflight = nullptr;
  int rc = 0;
  while (i < n && !rc) {
    if (lens[i] >= kMaxDev) {
      fallback.push_back(i++);
      continue;
    }
    size_t nh = 0, bytes = 0;
    while (i + nh < n && nh < MAX_CHUNK_HIST && lens[i + nh] < kMaxDev &&
           (nh == 0 || bytes + lens[i + nh] + 1 <= chunk)) {
      bytes += lens[i + nh] + 1;
      ++nh;
    }
    Slot& s = S.slot[k++ & 1];
    rc = launch_chunk(s, bufs, lens, i, nh, st, err);
    i += nh;
    if (!rc && inflight) rc = finish_chunk(*inflight, pre, on_device, fallback, st, err);
    inflight = rc ? nullptr : &s;
  }
  if (!rc && inflight) rc = finish_chunk(*inflight, pre, on_device, fallback, st, err);
  if (rc) return rc;
  st.n_fallback = (uint32_t)fallback.size();
  const int64_t t0 = steady_ns();
  auto one = [&](size_t j) {
    const size_t x = fallback[j];
    try {
      rcs[x] = load_jsonl_finalized(bufs[x], lens[x], pre[x]->h, errs[x]);
    } catch (...) {
      rcs[x] = S2LC_ENOMEM;
      errs[x] = "out of memory";
    }
  };
  if (n_threads == 1) {
    for (size_t j = 0; j < fallback.size(); ++j) one(j);
  } else {
    parallel_for(fallback.size(), 1, one);
  }
  st.load_ms += 1e-6 * (steady_ns() - t0);
  return 0;
}

}  // namespace s2lc
