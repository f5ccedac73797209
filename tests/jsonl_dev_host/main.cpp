// The device JSONL decoder's host-compilable core (csrc/jsonl_dev.h) driven
// serially, for the host sanitizers: each history is split at '\n' as the
// kernels split it, every record goes through jd::parse_record, the history
// through jd::seq_step, jd::finish_hist and jd::layout_*, and the result is
// compared with the CPU decoder (s2lc_load_jsonl): the accept / refuse
// decision, per-event fields, K, n_tokens, and the section bytes with
// s2lc_history_save_many's.
//
// usage: jsonl_dev_host [+|-|?]file ...
//   +file  the core must accept it      -file  the core must refuse it
//   ?file  either (what the CPU decoder refuses, the core must refuse)
// A few simulated histories (s2lc_simulate_jsonl) are always run first.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "jsonl_dev.h"
#include "s2lincheck.h"

using namespace s2lc;

static int g_fail = 0;
#define CHECK(c, ...)                      \
  do {                                     \
    if (!(c)) {                            \
      fprintf(stderr, "FAIL %s: ", name);  \
      fprintf(stderr, __VA_ARGS__);        \
      fprintf(stderr, "\n");               \
      ++g_fail;                            \
      return;                              \
    }                                      \
  } while (0)

struct Decoded {
  bool ok = false;
  std::vector<uint8_t> text;  // staged: a final '\n' appended where missing, then the zero pad
  std::vector<jd::Rec> recs;
  std::vector<uint32_t> hash_off, tokid;
  std::vector<jd::Op> ops;
  std::vector<jd::TokRef> toks;
  std::vector<uint32_t> cs;
  jd::Hist hi{};
  std::vector<uint64_t> sec;  // the section (8-byte aligned storage)
};

static void device_core(const uint8_t* buf, size_t len, Decoded& D) {
  D.text.assign(buf, buf + len);
  if (len && buf[len - 1] != '\n') D.text.push_back('\n');
  const uint32_t B = (uint32_t)D.text.size();
  D.text.resize(B + jd::TEXT_PAD, 0);
  std::vector<uint32_t> nl;
  for (uint32_t i = 0; i < B; ++i)
    if (D.text[i] == '\n') nl.push_back(i);
  const uint32_t n = (uint32_t)nl.size();
  D.recs.resize(n);
  D.hash_off.resize(n);
  bool all_ok = true;
  uint32_t carry = 0;
  for (uint32_t r = 0; r < n; ++r) {
    // the record in a buffer of exactly its size: a read outside [start, end) is a sanitizer report
    const uint32_t start = r ? nl[r - 1] + 1 : 0, end = nl[r];
    std::vector<uint8_t> one(D.text.begin() + start, D.text.begin() + end);
    jd::Rec a, b;
    const bool oka = jd::parse_record(one.data(), 0, end - start, a);
    const bool okb = jd::parse_record(D.text.data(), start, end, b);
    if (oka != okb) { fprintf(stderr, "parse_record depends on bytes outside the record\n"); exit(2); }
    D.recs[r] = b;
    all_ok = all_ok && okb;
    D.hash_off[r] = carry;
    carry += b.hash_cnt;
  }
  D.hi.rec_base = 0;
  D.hi.n_rec = n;
  D.tokid.assign(n, 0);
  D.ops.resize(n);
  D.toks.resize(jd::MAX_TOKENS);
  D.cs.assign(jd::MAX_CHAINS + 1, 0);
  std::vector<uint32_t> last(jd::MAX_CHAINS), chain_len(jd::MAX_CHAINS), open_op(jd::MAX_CHAINS);
  std::vector<uint32_t> tlen(jd::MAX_TOKENS);
  std::vector<uint64_t> tkey(jd::MAX_TOKENS);
  jd::Seq S;
  S.text = D.text.data();
  S.ops = D.ops.data();
  S.tokid = D.tokid.data();
  S.toks = D.toks.data();
  S.last = last.data();
  S.chain_len = chain_len.data();
  S.open_op = open_op.data();
  S.tkey = tkey.data();
  S.tlen = tlen.data();
  jd::HistOut out{};
  D.ok = all_ok;
  for (uint32_t r = 0; r < n && D.ok; ++r) D.ok = jd::seq_step(S, r, jd::seq_in(D.text.data(), D.recs[r]));
  D.ok = D.ok && jd::seq_finish(S, out);
  if (!D.ok) return;
  D.hi.ok = 1;
  jd::finish_hist(D.hi, out, carry, chain_len.data(), D.toks.data(), D.cs.data());
  D.sec.assign(D.hi.sec_size / 8, 0xA5A5A5A5A5A5A5A5ull);  // (every byte must be written)
  const jd::Layout L{D.text.data(), D.recs.data(), D.ops.data(), D.tokid.data(), D.hash_off.data(), D.cs.data(),
                     D.toks.data(), reinterpret_cast<uint8_t*>(D.sec.data())};
  const uint32_t nt = 7;  // lanes, serially: any interleaving of the fills gives the same bytes
  uint32_t n_ident = 0;
  for (uint32_t t = nt; t-- > 0;) n_ident += jd::layout_fill(L, D.hi, t, nt);
  jd::layout_head(L, D.hi, n_ident);
  D.hi.n_ident = n_ident;
  for (uint32_t t = 0; t < nt; ++t) jd::layout_sufmin(L, D.hi, t, nt);
}

static bool str_eq(const char* s, const uint8_t* text, uint32_t off, uint32_t len) {
  return s && strlen(s) == len && memcmp(s, text + off, len) == 0;
}

static void run_one(const char* name, const uint8_t* buf, size_t len, char expect) {
  Decoded D;
  device_core(buf, len, D);
  s2lc_history* h = nullptr;
  char err[256] = {0};
  const int rc = s2lc_load_jsonl(nullptr, len ? buf : (const uint8_t*)"", len, &h, err, sizeof err);
  if (expect == '+') CHECK(D.ok, "the core refused a history it must accept");
  if (expect == '-') CHECK(!D.ok, "the core accepted a history it must refuse");
  if (rc) {
    CHECK(!D.ok, "the core accepted what the CPU decoder refuses (%s)", err);
    return;
  }
  struct Free {
    s2lc_history* h;
    ~Free() { s2lc_history_free(h); }
  } fr{h};
  if (!D.ok) return;
  s2lc_history_info info;
  CHECK(s2lc_history_info_get(h, &info) == 0, "info");
  CHECK(info.n_events == D.hi.n_rec, "n_events %u != %u", D.hi.n_rec, info.n_events);
  CHECK(info.n_ops == D.hi.n_ops, "n_ops %u != %u", D.hi.n_ops, info.n_ops);
  CHECK(info.n_chains == D.hi.K, "K %u != %u", D.hi.K, info.n_chains);
  CHECK(info.n_tokens == D.hi.n_tokens, "n_tokens %u != %u", D.hi.n_tokens, info.n_tokens);
  CHECK(info.n_record_hashes == D.hi.n_pool, "n_pool");
  CHECK(info.n_identity_ops == D.hi.n_ident, "n_ident %u != %u", D.hi.n_ident, info.n_identity_ops);
  CHECK(info.structural == 0, "structural");
  std::vector<s2lc_event> ev(info.n_events);
  CHECK(s2lc_history_get_events(h, ev.data(), ev.size()) == 0, "get_events");
  const uint8_t* text = D.text.data();
  std::vector<uint64_t> hs;
  for (uint32_t i = 0; i < info.n_events; ++i) {
    const jd::Rec& r = D.recs[i];
    const s2lc_event& e = ev[i];
    CHECK(e.kind == r.kind && e.op_id == r.op_id && e.client_id == r.client_id, "event %u: kind / ids", i);
    if (r.kind == 0) {
      CHECK(e.input_type == r.input_type && e.has_num_records == (r.input_type == 0) &&
                e.has_match_seq_num == !!(r.bits & jd::RB_HAS_MSN) && e.num_records == r.a && e.match_seq_num == r.b,
            "event %u: call fields", i);
      CHECK(e.n_record_hashes == r.hash_cnt, "event %u: hash count", i);
      hs.assign(r.hash_cnt, 0);
      jd::convert_hashes(text, r, hs.data());
      CHECK(!r.hash_cnt || memcmp(hs.data(), e.record_hashes, 8ull * r.hash_cnt) == 0, "event %u: hashes", i);
      CHECK((r.bits & jd::RB_HAS_SET) ? str_eq(e.set_fencing_token, text, r.set_off, r.set_len) : !e.set_fencing_token,
            "event %u: set_fencing_token", i);
      CHECK((r.bits & jd::RB_HAS_TOK) ? str_eq(e.fencing_token, text, r.tok_off, r.tok_len) : !e.fencing_token,
            "event %u: fencing_token", i);
    } else {
      CHECK(e.failure == !!(r.bits & jd::RB_FAIL) && e.definite_failure == !!(r.bits & jd::RB_DEF) &&
                e.has_tail == !!(r.bits & jd::RB_HAS_TAIL) && e.has_stream_hash == !!(r.bits & jd::RB_HAS_HASH) &&
                e.tail == r.a && e.stream_hash == r.b,
            "event %u: return fields", i);
    }
  }
  uint8_t* img = nullptr;
  size_t img_len = 0;
  const s2lc_history* one[1] = {h};
  CHECK(s2lc_history_save_many(one, 1, &img, &img_len) == 0, "save_many");
  const size_t head = 8 + 4 + 4 + 8 + 8 * 2;  // magic, version, sizeof(Event), n, off[2]
  const bool same = img_len == head + D.hi.sec_size && memcmp(img + head, D.sec.data(), D.hi.sec_size) == 0;
  size_t at = 0;
  if (!same && img_len == head + D.hi.sec_size)
    while (img[head + at] == reinterpret_cast<uint8_t*>(D.sec.data())[at]) ++at;
  s2lc_free(img);
  CHECK(same, "section differs from the cache image (%zu vs %zu bytes, first difference at %zu)",
        (size_t)D.hi.sec_size, img_len - head, at);
}

int main(int argc, char** argv) {
  int n = 0;
  for (uint32_t wf = 0; wf < 3; ++wf) {
    for (uint64_t seed = 0; seed < 4; ++seed) {
      s2lc_sim_params p;
      s2lc_sim_params_default(&p);
      p.workflow = wf;
      p.num_clients = 3 + (uint32_t)seed * 15;  // 3 .. 48 chains
      p.ops_per_client = 30;
      p.seed = 100 + seed;
      p.p_indefinite = 0.05;
      p.p_definite = 0.05;
      p.p_read_failure = 0.02;
      p.p_check_tail_failure = 0.02;
      uint8_t* buf = nullptr;
      size_t len = 0;
      if (s2lc_simulate_jsonl(&p, &buf, &len) != 0) { fprintf(stderr, "simulate failed\n"); return 2; }
      char name[64];
      snprintf(name, sizeof name, "sim wf=%u seed=%llu", wf, (unsigned long long)p.seed);
      run_one(name, buf, len, '+');
      s2lc_free(buf);
      ++n;
    }
  }
  for (int a = 1; a < argc; ++a) {
    const char expect = argv[a][0];
    const char* path = argv[a] + 1;
    if (expect != '+' && expect != '-' && expect != '?') { fprintf(stderr, "bad argument %s\n", argv[a]); return 2; }
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    std::vector<uint8_t> data;
    uint8_t tmp[1 << 16];
    size_t k;
    while ((k = fread(tmp, 1, sizeof tmp, f)) > 0) data.insert(data.end(), tmp, tmp + k);
    fclose(f);
    run_one(path, data.data(), data.size(), expect);
    ++n;
  }
  printf("jsonl_dev_host: %d histories, %d failures\n", n, g_fail);
  return g_fail ? 1 : 0;
}
