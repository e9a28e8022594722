// The batch planner (bialign_amd/csrc/bialign_plan.hpp) on the CPU.  Stand-alone program, host code only, no HIP call
// (tests/test_plan_host.py compiles and runs it; tests/test_gpu_plan_agrees.py compares the library's plans with its).
// It reads one request per line from stdin, `key=value` words in any order, and answers in lines that diff well.
//
//   env NAME=VALUE | env NAME=      set / unset an environment switch the planner reads (BIALIGN_TEAM, BIALIGN_SLIM, ...)
//   raw   ...                       a hand-filled plan: geometry, LDS needs, one chunk plan, team shapes -- only the
//                                   functions that exist under the same names since before the planner was split off
//   batch ...                       a whole creation: check_inputs, score_bound, plan_pairs, decide_pack, plan_storage
//                                   (null batches: expand_null_pairs first; replan=1: replan_full_layout afterwards)
// Shared words: s (max_shift), k1 k2, beta gamma delta, budget (bytes; batch: 0 = from `free`, the free HBM in bytes),
// num_cu resid resid8 (what team_shape is told of the device), quiet=1 (hashes instead of the per-pair and order lines), pairs=NxM,NxM*COUNT,...
//   raw:   affine dense dense1 feat lean pack (0/1)
//   batch: rec flags, form=lookup|mu1|mu2|mu12|feature, amax bmax (one entry of otherwise zero S1 / S2 tables), mu1 mu2 (the
//          constant of the dense tables), fa=up,down,unp fb=up,down,unp (one feature value per plane and side), sw,
//          replicas seed (null batch)
// Answer of a batch: `rc=<code> msg=<message>`, `mode=<0 global|1 fit|2 local> flags=<the flags the planner saw>`, and on
// success the plan as print_plan() writes it, a `size` line per pair, and for plans with a ring term (the wide-band affine
// sweep outside the LEVEL forms) a `ring` line per pair and `max_chunk_ring_dwords`.
#include "bialign_plan.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

using namespace bialign;

// ---- the error record
static char g_msg[512] = "";
namespace bialign {
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace bialign

// ---- requests
struct Request {
  std::map<std::string, std::string> kv;
  std::vector<std::pair<int, int>> pairs;
  long long num(const char* key, long long dflt = 0) const {
    auto it = kv.find(key);
    return it == kv.end() ? dflt : std::strtoll(it->second.c_str(), nullptr, 10);
  }
  std::string str(const char* key, const char* dflt = "") const {
    auto it = kv.find(key);
    return it == kv.end() ? dflt : it->second;
  }
  void triple(const char* key, double out[3]) const {
    std::string s = str(key, "0,0,0");
    for (char& c : s)
      if (c == ',') c = ' ';
    std::istringstream in(s);
    std::string w;
    for (int f = 0; f < 3 && (in >> w); ++f) out[f] = std::strtod(w.c_str(), nullptr);
  }
};

static Request parse(std::istringstream& in) {
  Request r;
  std::string word;
  while (in >> word) {
    const size_t eq = word.find('=');
    if (eq == std::string::npos) continue;
    const std::string key = word.substr(0, eq), val = word.substr(eq + 1);
    if (key != "pairs") {
      r.kv[key] = val;
      continue;
    }
    std::istringstream ps(val);
    std::string item;
    while (std::getline(ps, item, ',')) {
      int n = 0, m = 0, count = 1;
      if (std::sscanf(item.c_str(), "%dx%d*%d", &n, &m, &count) < 2) continue;
      for (int c = 0; c < count; ++c) r.pairs.emplace_back(n, m);
    }
  }
  return r;
}

static uint64_t mix(uint64_t h, int64_t v) { return (h ^ (uint64_t)v) * 1099511628211ull; }  // FNV-1a over whole values

// The plan, line by line: decisions, LDS, chunks, launch order, pairs, chunk maxima, and every chunk's team shape
static void print_plan(const BatchPlan& b, const Request& r) {
  const int storage = b.level_trace ? BIALIGN_BATCH_LEVEL_TRACE : (b.lean_trace ? BIALIGN_BATCH_LEAN_TRACE : (b.lean ? BIALIGN_BATCH_SCORE_ONLY : 0));
  std::printf("plan pack=%d packed_sizing=%d storage=%d resw_k=%d wide_seg=%d cells=%lld trace_bytes=%lld\n", (int)b.pack,
              (int)b.packed_sizing, storage, b.resw_k, b.wide_seg, (long long)b.cells, (long long)b.trace_bytes);
  std::printf("lds bytes=%zu base=%zu per_wave=%zu diet8=%zu slim_base=%zu slim_codes=%zu trace=%zu\n", b.lds_bytes, b.lds_base,
              b.lds_per_wave, b.lds_diet8, b.lds_slim_base, b.lds_slim_codes, b.lds_trace);
  std::printf("chunks");
  for (int c : b.chunk_begin) std::printf(" %d", c);
  std::printf("\n");
  if (r.num("quiet")) {
    uint64_t ho = 14695981039346656037ull, hp = ho;
    for (int32_t o : b.order) ho = mix(ho, o);
    for (const PairDesc& d : b.pairs)
      for (int64_t v : {(int64_t)d.NS, (int64_t)d.P, (int64_t)d.G, d.layer_off, d.scratch_off, d.tab_off}) hp = mix(hp, v);
    std::printf("order_hash %016llx\npairs_hash %016llx\n", (unsigned long long)ho, (unsigned long long)hp);
  } else {
    std::printf("order");
    for (int32_t o : b.order) std::printf(" %d", o);
    std::printf("\n");
    for (size_t p = 0; p < b.pairs.size(); ++p) {
      const PairDesc& d = b.pairs[p];
      std::printf("pair %zu NS=%d P=%d G=%d layer_off=%lld scratch_off=%lld tab_off=%lld\n", p, d.NS, d.P, d.G, (long long)d.layer_off,
                  (long long)d.scratch_off, (long long)d.tab_off);
    }
  }
  std::printf("max_chunk_dwords=%lld max_chunk_tab_dwords=%lld\n", (long long)b.max_chunk_dwords, (long long)b.max_chunk_tab_dwords);
  // (plans with a ring term only -- the wide-band affine sweep outside the LEVEL forms: the ring area of the largest chunk)
  if (!b.ring_dwords.empty()) std::printf("max_chunk_ring_dwords=%lld\n", (long long)b.max_chunk_ring_dwords);
  for (size_t c = 0; !b.wide && c + 1 < b.chunk_begin.size(); ++c) {
    const int first = b.chunk_begin[c], count = b.chunk_begin[c + 1] - first;
    const TeamShape ts = team_shape(b, first, count, (int)r.num("num_cu", 256), (int)r.num("resid"), (int)r.num("resid8"));
    std::printf("team chunk=%zu tw=%d gw=%d slim=%d\n", c, ts.tw, ts.gw, (int)ts.slim);
  }
}

// ---- a hand-filled plan of a tiled batch: sweep_geometry, cells_of, lds_need*, plan_chunks, team_shape
static void run_raw(const Request& r) {
  BatchPlan b;
  b.affine = (int)r.num("affine", 1);
  b.NL = b.affine ? 9 : 1;
  b.S = (int)r.num("s", 1);
  b.k1 = (int)r.num("k1", 20), b.k2 = (int)r.num("k2", 3);
  b.prm.gap_opening_cost = (int32_t)r.num("beta", -150);
  b.dense = r.num("dense") || r.num("feat"), b.dense1 = r.num("dense1"), b.feat = r.num("feat");
  b.lean = r.num("lean"), b.pack = r.num("pack");
  b.npairs = (int)r.pairs.size();
  b.pairs.resize(b.npairs);
  const SweepInfo& geo = sweep_info(b);
  const LdsForm form{b.dense, false, b.dense1}, diet{false, true, false};
  std::vector<int64_t> dwords(b.npairs);
  for (int p = 0; p < b.npairs; ++p) {
    PairDesc& d = b.pairs[p];
    d = PairDesc{};
    d.n = r.pairs[p].first, d.m = r.pairs[p].second;
    sweep_geometry(geo, d.n, d.m, &d.NS, &d.P, &d.G);
    b.cells += cells_of(d.n, d.m, b.S);
    b.lds_bytes = std::max(b.lds_bytes, lds_need(geo, 1, b.k1, b.k2, d.n, d.m, form));
    b.lds_base = std::max(b.lds_base, lds_need(geo, 0, b.k1, b.k2, d.n, d.m, form));
    b.lds_diet8 = std::max(b.lds_diet8, lds_need(geo, 8, b.k1, b.k2, d.n, d.m, diet));
    b.lds_slim_codes = std::max(b.lds_slim_codes, lds_need_slim_codes(geo, d.n, d.m));
    if (b.feat) b.tab_dwords.push_back((int64_t)d.n * d.m);
    dwords[p] = (int64_t)d.G * (b.lean ? geo.lean_recdw : geo.recdw);
  }
  b.lds_per_wave = lds_need(geo, 1, b.k1, b.k2, 1, 1, form) - lds_need(geo, 0, b.k1, b.k2, 1, 1, form);
  b.lds_slim_base = lds_need_slim_base(geo, b.k1, b.k2);
  g_msg[0] = 0;
  const int rc = plan_chunks(b, dwords, r.num("budget", 1ll << 40) / 4);
  std::printf("rc=%d msg=%s\n", rc, g_msg);
  if (rc == BIALIGN_OK) print_plan(b, r);
}

// ---- a whole creation, as create_batch() orders it (bialign_capi.hip), without the device
static void run_batch(const Request& r) {
  const std::string form = r.str("form", "lookup");
  const bool feature = form == "feature", dense1 = form == "mu1" || form == "mu12", dense2 = form == "mu2" || form == "mu12";
  bialign_params prm{};
  prm.max_shift = (int32_t)r.num("s", 1);
  prm.recurrence = (int32_t)r.num("rec", BIALIGN_REC_AUTO);
  prm.flags = (uint32_t)r.num("flags");
  prm.gap_opening_cost = (int32_t)r.num("beta", -150), prm.gap_cost = (int32_t)r.num("gamma", -50), prm.shift_cost = (int32_t)r.num("delta", -150);
  bialign_scoring sc{};
  sc.k1 = (int32_t)r.num("k1", 20), sc.k2 = (int32_t)r.num("k2", 3);
  std::vector<int32_t> s1((size_t)std::max(sc.k1, 1) * std::max(sc.k1, 1), 0), s2((size_t)std::max(sc.k2, 1) * std::max(sc.k2, 1), 0);
  s1[0] = (int32_t)r.num("amax"), s2[0] = (int32_t)r.num("bmax");
  sc.s1 = s1.data(), sc.s2 = s2.data();

  const int np = (int)r.pairs.size();
  std::vector<int32_t> len_a(np), len_b(np);
  std::vector<int64_t> off_a(np), off_b(np), tab_off(np);
  int64_t tot_a = 0, tot_b = 0, tot_tab = 0;
  for (int p = 0; p < np; ++p) {  // every pair its own two molecules, end to end
    len_a[p] = r.pairs[p].first, len_b[p] = r.pairs[p].second;
    off_a[p] = tot_a, off_b[p] = tot_b, tab_off[p] = tot_tab;
    tot_a += std::max(len_a[p], 0), tot_b += std::max(len_b[p], 0), tot_tab += (int64_t)std::max(len_a[p], 0) * std::max(len_b[p], 0);
  }
  std::vector<uint8_t> codes((size_t)std::max(tot_a, tot_b) + 1, 0);
  std::vector<int32_t> mu1((size_t)(dense1 ? tot_tab : 0), (int32_t)r.num("mu1")), mu2((size_t)(dense2 ? tot_tab : 0), (int32_t)r.num("mu2"));
  bialign_pairs pr{};
  pr.npairs = np;
  pr.len_a = len_a.data(), pr.len_b = len_b.data(), pr.off_a = off_a.data(), pr.off_b = off_b.data();
  pr.seq_a = pr.seq_b = pr.cls_a = pr.cls_b = codes.data();
  if (dense1) pr.mu1_dense = mu1.data(), pr.mu1_off = tab_off.data();
  if (dense2) pr.mu2_dense = mu2.data(), pr.mu2_off = tab_off.data();
  double fa[3] = {0, 0, 0}, fb[3] = {0, 0, 0};
  r.triple("fa", fa), r.triple("fb", fb);
  std::vector<double> plane_a[3], plane_b[3];
  bialign_features ft{};
  if (feature) {
    for (int f = 0; f < 3; ++f) plane_a[f].assign((size_t)tot_a + 1, fa[f]), plane_b[f].assign((size_t)tot_b + 1, fb[f]);
    ft.structure_weight = (int32_t)r.num("sw", 400);
    ft.up_a = plane_a[0].data(), ft.down_a = plane_a[1].data(), ft.unp_a = plane_a[2].data();
    ft.up_b = plane_b[0].data(), ft.down_b = plane_b[1].data(), ft.unp_b = plane_b[2].data();
  }

  g_msg[0] = 0;
  BatchPlan b;
  NullPlan nul{};
  const int R = (int)r.num("replicas");
  const bialign_params* uprm = &prm;
  const bialign_pairs* upr = &pr;
  int rc = BIALIGN_OK;
  if (R) {
    rc = expand_null_pairs(&prm, &pr, feature ? &ft : nullptr, R, (uint32_t)r.num("seed"), dense1 || dense2, nul);
    uprm = &nul.vprm, upr = &nul.vp;
  }
  const NullPlan* unul = R ? &nul : nullptr;
  const bialign_features* uft = feature ? &ft : nullptr;
  int64_t colmax = 0;
  if (rc == BIALIGN_OK) rc = check_inputs(uprm, &sc, upr, uft, unul, b);
  if (rc == BIALIGN_OK) rc = score_bound(uprm, &sc, upr, uft, unul, b, &colmax);
  if (rc == BIALIGN_OK) rc = plan_pairs(upr, unul, colmax, b);
  if (rc == BIALIGN_OK) {
    decide_pack(b, colmax);
    rc = plan_storage(b, budget_dwords(r.num("budget"), (size_t)r.num("free", 1ll << 40)));
  }
  std::printf("rc=%d msg=%s\nmode=%d flags=%u\n", rc, g_msg, (int)b.mode, (unsigned)b.prm.flags);
  if (rc != BIALIGN_OK) return;
  std::printf("colmax=%lld npairs=%d tot_a=%lld tot_b=%lld tot_tab=%lld\n", (long long)colmax, b.npairs, (long long)b.tot_a,
              (long long)b.tot_b, (long long)b.tot_tab);
  print_plan(b, r);
  for (int p = 0; p < b.npairs && !r.num("quiet"); ++p)  // what a pair takes inside the budget, and in its full-record form
    std::printf("size %d dwords=%lld tab_dwords=%lld full_dwords=%lld\n", p, (long long)b.pair_dwords[p],
                (long long)(b.tab_scratch() ? b.tab_dwords[p] : 0), (long long)b.full_dwords[p]);
  for (int p = 0; p < b.npairs && !b.ring_dwords.empty() && !r.num("quiet"); ++p)  // ... and its ring, where the plan has that term
    std::printf("ring %d ring_dwords=%lld ring_off=%lld\n", p, (long long)b.ring_dwords[p], (long long)b.pairs[p].scratch_off);
  if (r.num("replan") && b.packed_sizing) {  // as replan_full() does: within the buffers the first plan sized
    const int64_t layer_cap = std::max(b.max_chunk_dwords, *std::max_element(b.full_dwords.begin(), b.full_dwords.end()));
    const int64_t tab_cap = b.max_chunk_tab_dwords;
    b.pack_failed = true;
    rc = replan_full_layout(b, layer_cap, tab_cap);
    std::printf("replan rc=%d layer_cap=%lld tab_cap=%lld msg=%s\n", rc, (long long)layer_cap, (long long)tab_cap, rc ? g_msg : "");
    if (rc == BIALIGN_OK) print_plan(b, r);
  }
}

int main() {
  std::string line;
  int cases = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    if (!(in >> kind) || kind[0] == '#') continue;
    if (kind == "env") {
      std::string word;
      in >> word;
      const size_t eq = word.find('=');
      if (eq == std::string::npos) continue;
      if (eq + 1 == word.size()) unsetenv(word.substr(0, eq).c_str());
      else setenv(word.substr(0, eq).c_str(), word.c_str() + eq + 1, 1);
      std::printf("%s\n", line.c_str());
      continue;
    }
    const Request r = parse(in);
    std::printf("case %d: %s\n", cases++, line.c_str());
    if (kind == "raw") run_raw(r);
    else if (kind == "batch") run_batch(r);
    else std::printf("rc=-1 msg=unknown request\n");
  }
  return 0;
}
