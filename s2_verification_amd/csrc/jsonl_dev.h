// jsonl_dev.h — the core of the device JSONL decoder (jsonl_dev.hip), written
// so that the host compiles it too: the per-record parser, the per-history
// sequential pass and the section layout take a byte range and fill plain
// structs, and use no cross-lane operation. tests/jsonl_dev_host drives them
// serially under the host sanitizers and compares with s2lc_load_jsonl and
// s2lc_history_save_many.
//
// What they restate is jsonl.cpp's fast path, narrowed:
//   * parse_record = fast_parse on one record [start, end) that must be
//     consumed exactly (the caller splits the text at '\n'; a string cannot
//     hold one, so in an accepted history every '\n' is a record boundary);
//   * seq_step / seq_finish = load_direct's loop: op ids 0, 1, 2, ... in call
//     order, one Finish per op after its Start, every op returned, the online
//     greedy colouring, token interning in first-appearance order;
//   * finish_hist / layout_* = load_direct's chain-major layout as
//     write_section (cache.cpp) stores it in mode 0.
// Anything else is refused (false): the history then takes the CPU decoder,
// which owns every error message.
#pragma once
#include <stdint.h>

#include "model.h"

#define JD_HD __host__ __device__ inline

namespace s2lc {
namespace jd {

constexpr uint32_t MAX_CHAINS = 512;   // device caps: a history past them takes the CPU decoder
constexpr uint32_t MAX_TOKENS = 64;
constexpr uint32_t MAX_TOKEN_LEN = 64;
constexpr uint32_t TEXT_PAD = 16;      // zero bytes after the staged text

enum : uint8_t {  // Rec::bits
  RB_HAS_MSN = 0x1, RB_FAIL = 0x2, RB_DEF = 0x4, RB_HAS_TAIL = 0x8, RB_HAS_HASH = 0x10, RB_HAS_SET = 0x20,
  RB_HAS_TOK = 0x40,
};

// One parsed record. a/b: num_records/msn of a Start, tail/stream_hash of a
// Finish; a field the record text does not carry stays 0.
struct Rec {
  int64_t client_id, op_id;
  uint64_t a, b;
  uint32_t hash_cnt;   // len(record_hashes) (== num_records)
  uint32_t hash_text;  // offset of the first hash literal in the text
  uint32_t set_off, tok_off;  // token bytes in the text
  uint16_t set_len, tok_len;
  uint8_t kind, input_type, bits, ok;
};
static_assert(sizeof(Rec) == 56, "Rec layout");

struct Cur {
  const uint8_t* t;
  uint32_t i, end;
};

// the literal w (NUL-terminated) at the cursor
JD_HD bool lit(Cur& c, const char* w) {
  uint32_t i = c.i;
  for (; *w; ++w, ++i)
    if (i >= c.end || c.t[i] != (uint8_t)*w) return false;
  c.i = i;
  return true;
}
JD_HD bool peek(const Cur& c, char ch) { return c.i < c.end && c.t[c.i] == (uint8_t)ch; }

// A u64 literal as Fast::u64 takes it: 1..20 digits, no leading zero, at most
// 2^64 - 1, not followed by '.', 'e' or 'E'.
JD_HD bool u64lit(Cur& c, uint64_t& v) {
  const uint32_t s = c.i;
  uint32_t i = s;
  uint64_t r = 0;
  while (i < c.end) {
    const uint8_t d = c.t[i];
    if (d < '0' || d > '9') break;
    if (i - s >= 20) return false;
    const uint64_t x = d - '0';
    if (r > (~0ull - x) / 10) return false;
    r = r * 10 + x;
    ++i;
  }
  const uint32_t n = i - s;
  if (n == 0 || (n > 1 && c.t[s] == '0')) return false;
  if (i < c.end && (c.t[i] == '.' || c.t[i] == 'e' || c.t[i] == 'E')) return false;
  c.i = i;
  v = r;
  return true;
}
JD_HD bool i64lit(Cur& c, int64_t& v) {
  uint64_t u;
  if (!u64lit(c, u) || u > 0x7FFFFFFFFFFFFFFFull) return false;
  v = (int64_t)u;
  return true;
}

// null | "printable ASCII without \ and ", at most MAX_TOKEN_LEN bytes"
JD_HD bool opt_tok(Cur& c, bool& has, uint32_t& off, uint16_t& len) {
  if (lit(c, "null")) { has = false; return true; }
  if (!peek(c, '"')) return false;
  uint32_t i = c.i + 1;
  const uint32_t q = i;
  while (i < c.end && c.t[i] != '"') {
    const uint8_t b = c.t[i];
    if (b < 0x20 || b >= 0x80 || b == '\\') return false;
    ++i;
  }
  if (i >= c.end || i - q > MAX_TOKEN_LEN) return false;
  has = true;
  off = q;
  len = (uint16_t)(i - q);
  c.i = i + 1;
  return true;
}

// The record text[start, end), consumed exactly. Reads no byte outside it.
JD_HD bool parse_record(const uint8_t* text, uint32_t start, uint32_t end, Rec& e) {
  e = Rec{};
  Cur c{text, start, end};
  if (!lit(c, "{\"event\":{\"")) return false;
  if (lit(c, "Start\":")) {
    e.kind = 0;
    if (lit(c, "\"Read\"")) e.input_type = 1;            // S2LC_INPUT_READ
    else if (lit(c, "\"CheckTail\"")) e.input_type = 2;  // S2LC_INPUT_CHECK_TAIL
    else {
      if (!lit(c, "{\"Append\":{\"num_records\":")) return false;
      e.input_type = 0;
      if (!u64lit(c, e.a) || !lit(c, ",\"record_hashes\":[")) return false;
      e.hash_text = c.i;
      uint32_t cnt = 0;
      if (!peek(c, ']')) {
        for (;;) {
          uint64_t v;
          if (!u64lit(c, v)) return false;
          ++cnt;
          if (peek(c, ',')) { ++c.i; continue; }
          break;
        }
      }
      e.hash_cnt = cnt;
      bool hs = false, ht = false;
      if (!lit(c, "],\"set_fencing_token\":") || !opt_tok(c, hs, e.set_off, e.set_len)) return false;
      if (!lit(c, ",\"fencing_token\":") || !opt_tok(c, ht, e.tok_off, e.tok_len)) return false;
      if (!lit(c, ",\"match_seq_num\":")) return false;
      if (!lit(c, "null")) {
        if (!u64lit(c, e.b)) return false;
        e.bits |= RB_HAS_MSN;
      }
      if (!lit(c, "}}")) return false;
      if ((uint64_t)cnt != e.a) return false;  // (the general parser reports the mismatch)
      if (hs) e.bits |= RB_HAS_SET;
      if (ht) e.bits |= RB_HAS_TOK;
    }
  } else if (lit(c, "Finish\":")) {
    e.kind = 1;
    if (lit(c, "\"AppendDefiniteFailure\"")) e.bits |= RB_FAIL | RB_DEF;
    else if (lit(c, "\"AppendIndefiniteFailure\"")) e.bits |= RB_FAIL;
    else if (lit(c, "\"ReadFailure\"")) e.bits |= RB_FAIL | RB_DEF;
    else if (lit(c, "\"CheckTailFailure\"")) e.bits |= RB_FAIL | RB_DEF;
    else {
      e.bits |= RB_HAS_TAIL;
      if (lit(c, "{\"AppendSuccess\":{\"tail\":")) {
        if (!u64lit(c, e.a)) return false;
      } else if (lit(c, "{\"CheckTailSuccess\":{\"tail\":")) {
        if (!u64lit(c, e.a)) return false;
      } else if (lit(c, "{\"ReadSuccess\":{\"tail\":")) {
        e.bits |= RB_HAS_HASH;
        if (!u64lit(c, e.a) || !lit(c, ",\"stream_hash\":") || !u64lit(c, e.b)) return false;
      } else {
        return false;
      }
      if (!lit(c, "}}")) return false;
    }
  } else {
    return false;
  }
  if (!lit(c, "},\"client_id\":") || !i64lit(c, e.client_id) || !lit(c, ",\"op_id\":") || !i64lit(c, e.op_id) ||
      !lit(c, "}"))
    return false;
  if (c.i != end) return false;
  e.ok = 1;
  return true;
}

// The record hashes of a parsed append (hash_cnt literals from hash_text,
// which parse_record validated) into out[0, hash_cnt).
JD_HD void convert_hashes(const uint8_t* text, const Rec& e, uint64_t* out) {
  uint32_t i = e.hash_text;
  for (uint32_t k = 0; k < e.hash_cnt; ++k) {
    uint64_t r = 0;
    for (;; ++i) {
      const uint8_t d = text[i];
      if (d < '0' || d > '9') break;
      r = r * 10 + (d - '0');
    }
    ++i;  // ',' (or the ']' after the last one)
    out[k] = r;
  }
}

// OpRec flags of an op (history.h op_flags; s2Model.Step's cases, main.go:264-335)
JD_HD uint32_t flags_of(uint8_t input_type, uint8_t start_bits, uint8_t fin_bits) {
  const bool failure = fin_bits & RB_FAIL, definite = fin_bits & RB_DEF;
  uint32_t f = input_type & OPF_KIND_MASK;
  if (failure) f |= OPF_FAIL;
  if (definite) f |= OPF_DEF;
  if (fin_bits & RB_HAS_TAIL) f |= OPF_HAS_TAIL;
  if (fin_bits & RB_HAS_HASH) f |= OPF_HAS_HASH;
  if (start_bits & RB_HAS_MSN) f |= OPF_HAS_MSN;
  if (input_type == 0) {
    if (failure && definite) f |= OPF_CLS_E;
    else if (failure) f |= OPF_CLS_I;
    else f |= OPF_CLS_D | OPF_CONSTRAIN;
  } else {
    f |= OPF_CLS_E;
    if (!failure || (fin_bits & RB_HAS_HASH)) f |= OPF_CONSTRAIN;
  }
  return f;
}

struct Op {  // per dense op, from the sequential pass
  uint32_t call_ev, ret_ev, chain, pos;  // pos: index within its chain
};
struct TokRef {
  uint32_t off, len;  // the token's bytes in the text (its first appearance)
};
struct HistOut {
  uint32_t n_ops, K, n_tokens, max_chain_len, hflags;
};

// What the sequential pass reads of one record. The kernel stages a tile of
// these in LDS with all its lanes, so that the one lane that makes the pass
// waits for no global load.
struct SeqIn {
  uint64_t a;                 // num_records of a Start
  uint64_t set_key, tok_key;  // tok_key() of the tokens
  uint32_t op_lo;             // op id (bad when it does not fit)
  uint32_t set_off, tok_off;
  uint16_t set_len, tok_len;
  uint8_t kind, input_type, bits, bad;  // bad: not parsed, or an op id of 2^32 or more (no op can have one)
};
static_assert(sizeof(SeqIn) == 48, "SeqIn layout");

// A token's comparison key: its bytes when it has at most 8 (then key and
// length decide equality), else a hash (equal keys are then compared bytewise).
JD_HD uint64_t tok_key(const uint8_t* text, uint32_t off, uint32_t len) {
  uint64_t k = len <= 8 ? 0 : 0xcbf29ce484222325ull;
  for (uint32_t j = 0; j < len; ++j) {
    if (len <= 8) k |= (uint64_t)text[off + j] << (8 * j);
    else k = (k ^ text[off + j]) * 0x100000001b3ull;
  }
  return k;
}

JD_HD SeqIn seq_in(const uint8_t* text, const Rec& r) {
  SeqIn s{};
  s.bad = !r.ok || r.op_id < 0 || r.op_id > 0xFFFFFFFFll;
  if (s.bad) return s;
  s.a = r.a;
  s.op_lo = (uint32_t)r.op_id;
  s.kind = r.kind;
  s.input_type = r.input_type;
  s.bits = r.bits;
  if (r.bits & RB_HAS_SET) {
    s.set_off = r.set_off;
    s.set_len = r.set_len;
    s.set_key = tok_key(text, r.set_off, r.set_len);
  }
  if (r.bits & RB_HAS_TOK) {
    s.tok_off = r.tok_off;
    s.tok_len = r.tok_len;
    s.tok_key = tok_key(text, r.tok_off, r.tok_len);
  }
  return s;
}

// The sequential pass's state. last, chain_len and open_op [MAX_CHAINS], tkey
// and tlen [MAX_TOKENS] are the caller's (LDS in the kernel); ops[n_rec],
// tokid[n_rec] (set id << 16 | batch id, per record) and toks[MAX_TOKENS] are
// only written (global memory there), except for the bytes of a token longer
// than 8 whose key matched.
struct Seq {
  const uint8_t* text;
  Op* ops;
  uint32_t* tokid;
  TokRef* toks;
  uint32_t *last, *chain_len, *open_op;
  uint64_t* tkey;
  uint32_t* tlen;
  uint32_t m = 0, K = 0, returned = 0, n_tokens = 0;
  uint64_t total = 0;
  bool nowrap = true;
};

// token -> id (1-based, first appearance order); 0: over the cap
JD_HD uint32_t intern(Seq& S, uint64_t key, uint32_t off, uint32_t len) {
  for (uint32_t k = 0; k < S.n_tokens; ++k) {
    if (S.tlen[k] != len || S.tkey[k] != key) continue;
    if (len <= 8) return k + 1;
    const uint32_t o = S.toks[k].off;
    uint32_t j = 0;
    while (j < len && S.text[o + j] == S.text[off + j]) ++j;
    if (j == len) return k + 1;
  }
  if (S.n_tokens >= MAX_TOKENS) return 0;
  S.toks[S.n_tokens] = TokRef{off, len};
  S.tkey[S.n_tokens] = key;
  S.tlen[S.n_tokens] = len;
  return ++S.n_tokens;
}

// One record of load_direct's loop (event index ev). false: the history is refused.
JD_HD bool seq_step(Seq& S, uint32_t ev, const SeqIn& r) {
  if (r.bad) return false;
  uint32_t tk = 0;
  if (r.kind == 0) {
    if (r.op_lo != S.m) return false;  // dense id = op id
    uint32_t st = 0, bt = 0;
    if (r.bits & RB_HAS_SET) {
      st = intern(S, r.set_key, r.set_off, r.set_len);
      if (!st) return false;
    }
    if (r.bits & RB_HAS_TOK) {
      bt = intern(S, r.tok_key, r.tok_off, r.tok_len);
      if (!bt) return false;
    }
    tk = (st << 16) | bt;
    // the chain whose last op returned earliest, if that return precedes this call
    uint32_t c = EV_INF, best = EV_INF;
    for (uint32_t k = 0; k < S.K; ++k) {
      const uint32_t x = S.last[k];
      const bool lt = x < best;
      best = lt ? x : best;
      c = lt ? k : c;
    }
    if (c == EV_INF) {
      if (S.K >= MAX_CHAINS) return false;
      c = S.K++;
      S.chain_len[c] = 0;
    }
    S.ops[S.m] = Op{ev, EV_INF, c, S.chain_len[c]};
    S.chain_len[c]++;
    S.last[c] = EV_INF;  // open: op m is its chain's last op until it returns
    S.open_op[c] = S.m;
    if (r.input_type == 0) {
      if (r.a > (1ull << 63) - S.total) S.nowrap = false;
      else S.total += r.a;
    }
    ++S.m;
  } else {
    if (r.op_lo >= S.m) return false;
    // its chain: the one it holds open (none: a second Finish)
    uint32_t c = EV_INF;
    for (uint32_t k = 0; k < S.K; ++k)
      if (S.last[k] == EV_INF && S.open_op[k] == r.op_lo) c = k;
    if (c == EV_INF) return false;
    S.ops[r.op_lo].ret_ev = ev;
    S.last[c] = ev;
    S.returned++;
  }
  S.tokid[ev] = tk;
  return true;
}

JD_HD bool seq_finish(const Seq& S, HistOut& out) {
  if (S.returned != S.m) return false;
  uint32_t mcl = 0;
  for (uint32_t k = 0; k < S.K; ++k) mcl = S.chain_len[k] > mcl ? S.chain_len[k] : mcl;
  out.n_ops = S.m;
  out.K = S.K;
  out.n_tokens = S.n_tokens;
  out.max_chain_len = mcl;
  uint32_t hf = 0x4 | 0x8;                               // H_P4 | H_IDEFER
  if (S.nowrap) hf |= 0x1 | 0x2;                         // H_NOWRAP | H_P2OK
  if (S.nowrap && S.total <= 0xFFFFFFFCull) hf |= 0x10;  // H_TAIL32
  out.hflags = hf;
  return true;
}

// The required pre-tail of a constraining op (load_direct's sufmin term).
JD_HD uint64_t req_of(uint32_t flags, uint64_t num_records, uint64_t out_tail) {
  uint64_t req;
  if ((flags & OPF_KIND_MASK) == 0) req = out_tail >= num_records ? out_tail - num_records : 0;
  else if (!(flags & OPF_FAIL)) req = out_tail;
  else req = REQ_HASH_ONLY;
  return req > REQ_HASH_ONLY ? REQ_HASH_ONLY : req;
}

// One history of a chunk: its records [rec_base, rec_base + n_rec) of the
// chunk's record list, and what the sequential pass found (ok = 0: refused).
// (n_ident is the layout's to count: the kernels leave the field 0.)
struct Hist {
  uint32_t rec_base, n_rec, ok, n_ops, K, n_tokens, n_ident, mcl, hflags, n_pool, tok_bytes, pad_;
  uint64_t sec_size;
};

JD_HD uint64_t pad8(uint64_t x) { return (x + 7) & ~(uint64_t)7; }

// After seq_finish accepted: the chain starts cs[K + 1] (each chain followed by
// its sentinel), the token bytes and the section's size (cache.cpp section_bytes).
JD_HD void finish_hist(Hist& hi, const HistOut& out, uint32_t n_pool, const uint32_t* chain_len, const TokRef* toks,
                       uint32_t* cs) {
  uint32_t pos = 0;
  for (uint32_t c = 0; c < out.K; ++c) {
    cs[c] = pos;
    pos += chain_len[c] + 1;
  }
  cs[out.K] = pos;
  uint32_t tb = 0;
  for (uint32_t t = 0; t < out.n_tokens; ++t) tb += (uint32_t)pad8(4 + toks[t].len);
  hi.n_ops = out.n_ops;
  hi.K = out.K;
  hi.n_tokens = out.n_tokens;
  hi.mcl = out.max_chain_len;
  hi.hflags = out.hflags;
  hi.n_pool = n_pool;
  hi.tok_bytes = tb;
  const uint64_t nr = (uint64_t)out.n_ops + out.K;
  hi.sec_size = sizeof(CacheHead) + 8ull * hi.n_rec + 8ull * n_pool + tb + pad8(4ull * (out.K + 1)) + 64ull * nr +
                pad8(4ull * nr) + 8ull * out.n_ops;
}

// The section of one accepted history as write_section (cache.cpp) lays it
// out in mode 0, written by nt cooperating lanes (this one is tid): fill
// (returns the lane's count of identity-class ops; their sum is n_ident),
// then — after every lane's fill is visible — head (one lane) and sufmin. recs, ops, tokid and
// hash_off are the history's own (already offset by rec_base); sec is 8-byte
// aligned with hi.sec_size bytes.
struct Layout {
  const uint8_t* text;
  const Rec* recs;
  const Op* ops;
  const uint32_t* tokid;
  const uint32_t* hash_off;
  const uint32_t* cs;
  const TokRef* toks;
  uint8_t* sec;
};
struct LayoutPtrs {
  int64_t* client;
  uint64_t* pool;
  uint8_t* tok;
  uint32_t* cs;
  uint64_t* recs;  // OpRec[n_ops + K] as 8 words each (a section is only 8-byte aligned; OpRec asks for 64)
  uint32_t* rec_op;
  int64_t* ids;
};
JD_HD LayoutPtrs layout_ptrs(uint8_t* sec, const Hist& hi) {
  const uint32_t nr = hi.n_ops + hi.K;
  LayoutPtrs p;
  p.client = reinterpret_cast<int64_t*>(sec + sizeof(CacheHead));
  p.pool = reinterpret_cast<uint64_t*>(p.client + hi.n_rec);
  p.tok = reinterpret_cast<uint8_t*>(p.pool + hi.n_pool);
  p.cs = reinterpret_cast<uint32_t*>(p.tok + hi.tok_bytes);
  p.recs = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(p.cs) + pad8(4ull * (hi.K + 1)));
  p.rec_op = reinterpret_cast<uint32_t*>(p.recs + 8ull * nr);
  p.ids = reinterpret_cast<int64_t*>(reinterpret_cast<uint8_t*>(p.rec_op) + pad8(4ull * nr));
  return p;
}

JD_HD void layout_head(const Layout& L, const Hist& hi, uint32_t n_ident) {
  const uint32_t nr = hi.n_ops + hi.K;
  CacheHead hd{0, 0, hi.n_ops, n_ident, hi.K, hi.hflags, hi.mcl, hi.n_tokens, hi.n_rec, hi.n_pool, nr, 0,
               (uint64_t)hi.K + 1};
  *reinterpret_cast<CacheHead*>(L.sec) = hd;
}

JD_HD uint32_t layout_fill(const Layout& L, const Hist& hi, uint32_t tid, uint32_t nt) {
  const uint32_t n = hi.n_rec, m = hi.n_ops, K = hi.K, nr = m + K;
  const LayoutPtrs P = layout_ptrs(L.sec, hi);
  uint32_t n_ident = 0;
  if (tid == 0) {
    uint8_t* p = P.tok;
    for (uint32_t t = 0; t < hi.n_tokens; ++t) {
      const uint32_t len = L.toks[t].len, tot = (uint32_t)pad8(4 + len);
      *reinterpret_cast<uint32_t*>(p) = len;
      for (uint32_t j = 0; j < len; ++j) p[4 + j] = L.text[L.toks[t].off + j];
      for (uint32_t j = 4 + len; j < tot; ++j) p[j] = 0;
      p += tot;
    }
    if ((K + 1) & 1) P.cs[K + 1] = 0;  // the u32 arrays' zero pad to 8 bytes
    if (nr & 1) P.rec_op[nr] = 0;
  }
  for (uint32_t e = tid; e < n; e += nt) {
    const Rec& r = L.recs[e];
    P.client[e] = r.client_id;
    if (r.hash_cnt) convert_hashes(L.text, r, P.pool + L.hash_off[e]);
  }
  for (uint32_t c = tid; c <= K; c += nt) P.cs[c] = L.cs[c];
  for (uint32_t d = tid; d < m; d += nt) {
    const Op op = L.ops[d];
    const Rec& s = L.recs[op.call_ev];
    const Rec& f = L.recs[op.ret_ev];
    const uint32_t tk = L.tokid[op.call_ev];
    const uint32_t flags = flags_of(s.input_type, s.bits, f.bits);
    n_ident += (flags & OPF_CLS_E) ? 1u : 0u;
    const uint32_t q = L.cs[op.chain] + op.pos;
    uint64_t* w = P.recs + 8ull * q;  // OpRec's fields in order (model.h; little endian)
    w[0] = s.a;  // num_records
    w[1] = s.b;  // msn
    w[2] = f.a;  // out_tail
    w[3] = f.b;  // out_hash
    // (sufmin: its own term for now, layout_sufmin turns it into the chain's suffix minimum)
    w[4] = (flags & OPF_CONSTRAIN) ? req_of(flags, s.a, f.a) : REQ_NONE;
    w[5] = (uint64_t)op.call_ev | ((uint64_t)op.ret_ev << 32);
    // (hash_off: the pool's size at an append, 0 for the other kinds, as fast_parse leaves it)
    w[6] = (uint64_t)(s.input_type == 0 ? L.hash_off[op.call_ev] : 0u) | ((uint64_t)s.hash_cnt << 32);
    w[7] = (uint64_t)(tk & 0xFFFF) | ((uint64_t)(tk >> 16) << 16) | ((uint64_t)flags << 32);  // batch_tok, set_tok, flags
    P.rec_op[q] = d;
    P.ids[d] = (int64_t)d;
  }
  for (uint32_t c = tid; c < K; c += nt) {
    const uint32_t q = L.cs[c + 1] - 1;
    uint64_t* w = P.recs + 8ull * q;  // all zero but call_ev = ret_ev = EV_INF, flags, sufmin
    w[0] = w[1] = w[2] = w[3] = w[6] = 0;
    w[4] = REQ_NONE;
    w[5] = ~0ull;
    w[7] = (uint64_t)OPF_SENTINEL << 32;
    P.rec_op[q] = EV_INF;
  }
  return n_ident;
}

JD_HD void layout_sufmin(const Layout& L, const Hist& hi, uint32_t tid, uint32_t nt) {
  const LayoutPtrs P = layout_ptrs(L.sec, hi);
  for (uint32_t c = tid; c < hi.K; c += nt) {
    uint64_t run = REQ_NONE;
    for (uint32_t x = L.cs[c + 1] - 1; x-- > L.cs[c];) {
      const uint64_t v = P.recs[8ull * x + 4];
      run = v < run ? v : run;
      P.recs[8ull * x + 4] = run;
    }
  }
}

}  // namespace jd

// ---- host interface of jsonl_dev.hip ----
struct JdStats {
  uint32_t n_device = 0, n_fallback = 0, n_rejected = 0;
  uint64_t bytes_in = 0, bytes_out = 0;
  double stage_ms = 0, h2d_ms = 0, kernel_ms = 0, d2h_ms = 0, load_ms = 0;
};
struct JdState;  // the context's grow-only stage and device buffers
void jd_release(JdState* s);

}  // namespace s2lc
