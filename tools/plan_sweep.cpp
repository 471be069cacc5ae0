// Walks the tick planner over EVERY batch size: wbc_plan_tick for N = 1 .. 2^21 in 64 configurations (2 scalar types x observer off / on x with / without
// M, h, Jc x cold / warm x 4 option sets), through include/wbc_hip.h alone.  No device, no HIP: it is built with the planner's two units alone (tools/Makefile),
// which is the proof that the planner needs neither.
//   plan_sweep           one line per configuration: the thresholds wbc_dispatch_thresholds reports, the number of runs of equal plans, and a 64-bit
//                        hash over every (N, plan) at which the plan changes -- two builds plan alike exactly when their 64 lines are equal
//   plan_sweep --check   also exits 1 unless, in every configuration, the reported thresholds are exactly the switch points found by brute force under
//                        the function's own rule: fp64 plans are compared with their neighbour (N with plan(N - 1) != plan(N)), fp32 plans even with
//                        even (even N >= 4 with plan(N - 2) != plan(N): an odd batch never packs); an odd reported threshold r of an fp32 configuration
//                        stands for the even switch r + 1.  The one-round tile SIZE (qp_tile) is not a switch and is left out of that comparison.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "wbc_hip.h"

static const size_t N_MAX = (size_t)1 << 21;

struct Config { int dtype, observer, mats, warm, optset; };
static const char* OPTSET[4] = {"defaults", "tile_tick=-1", "fused_pair=-1", "qp_lane=-1,qp_tile=-1,fused_max=0"};

static void options_of(int optset, wbc_solver_options* o) {
  wbc_solver_options_default(o);
  if (optset == 1) o->tile_tick = -1;
  if (optset == 2) o->fused_pair = -1;
  if (optset == 3) { o->qp_lane = -1; o->qp_tile = -1; o->fused_max = 0; }
}

struct Plan { int f[8]; };   // fused front qp qp_tile qp_body sweep_pack2 sweep_block qp_warm
static bool plan_of(const Config& c, const wbc_solver_options* o, size_t N, Plan* p) {
  wbc_tick_plan t;
  t.struct_size = sizeof(t);
  if (wbc_plan_tick(c.dtype, c.observer, o, N, c.mats, 1, c.warm, &t) != WBC_OK) return false;
  const int f[8] = {t.fused, t.front, t.qp, t.qp_tile, t.qp_body, t.sweep_pack2, t.sweep_block, t.qp_warm};
  std::memcpy(p->f, f, sizeof(f));
  return true;
}
static bool same_all(const Plan& a, const Plan& b) { return std::memcmp(a.f, b.f, sizeof(a.f)) == 0; }
static bool same_family(const Plan& a, const Plan& b) {   // every field but qp_tile
  for (int i = 0; i < 8; ++i) if (i != 3 && a.f[i] != b.f[i]) return false;
  return true;
}
static void hash_word(uint64_t& h, uint64_t w) {   // FNV-1a over the word's eight bytes
  for (int i = 0; i < 8; ++i) { h ^= (w >> (8 * i)) & 0xff; h *= 0x100000001b3ull; }
}

// one configuration: its output line, and whether the reported thresholds are the brute-force switch points
static bool sweep(const Config& c, std::string* line) {
  wbc_solver_options o;
  options_of(c.optset, &o);
  size_t th[64];
  int nth = 0;
  const int flags = (c.mats ? WBC_PLAN_WITH_MATS : 0) | (c.warm ? WBC_PLAN_WARM : 0);
  bool ok = wbc_dispatch_thresholds(c.dtype, c.observer, &o, flags, th, 64, &nth) == WBC_OK && nth <= 64;
  std::vector<size_t> reported, found;
  for (int i = 0; ok && i < nth; ++i) reported.push_back((c.dtype == WBC_F32 && th[i] % 2 == 1) ? th[i] + 1 : th[i]);
  uint64_t h = 0xcbf29ce484222325ull;
  size_t runs = 0;
  Plan prev{}, prev2{}, cur{};   // plan(N - 1), plan(N - 2), plan(N)
  for (size_t N = 1; ok && N <= N_MAX; ++N) {
    ok = plan_of(c, &o, N, &cur);
    if (N == 1 || !same_all(prev, cur)) {
      ++runs;
      hash_word(h, N);
      for (int v : cur.f) hash_word(h, (uint64_t)(int64_t)v);
    }
    if (N >= 2) {
      if (c.dtype == WBC_F64) { if (!same_family(prev, cur)) found.push_back(N); }
      else if (N % 2 == 0 && N >= 4 && !same_family(prev2, cur)) found.push_back(N);   // (from 4: plan(0) is no batch's plan)
    }
    prev2 = prev; prev = cur;
  }
  ok = ok && reported == found;
  char buf[256];
  std::snprintf(buf, sizeof(buf), "%s obs=%d mats=%d warm=%d [%s]: thresholds", c.dtype == WBC_F64 ? "f64" : "f32", c.observer, c.mats, c.warm, OPTSET[c.optset]);
  *line = buf;
  for (int i = 0; i < nth && i < 64; ++i) *line += " " + std::to_string(th[i]);
  std::snprintf(buf, sizeof(buf), " | runs %zu | hash %016llx", runs, (unsigned long long)h);
  *line += buf;
  if (!ok) {
    *line += " | MISMATCH, brute-force switches:";
    for (size_t n : found) *line += " " + std::to_string(n);
  }
  return ok;
}

int main(int argc, char** argv) {
  const bool check = argc > 1 && std::strcmp(argv[1], "--check") == 0;
  std::vector<Config> cfg;
  for (int dtype : {WBC_F64, WBC_F32})
    for (int observer : {0, 1})
      for (int mats : {1, 0})
        for (int warm : {0, 1})
          for (int optset = 0; optset < 4; ++optset) cfg.push_back({dtype, observer, mats, warm, optset});
  std::vector<std::string> lines(cfg.size());
  std::vector<char> good(cfg.size(), 0);
  std::atomic<size_t> next{0};
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt < 1 ? 1 : (nt > 16 ? 16 : nt);
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < nt; ++t)
    pool.emplace_back([&] { for (size_t i; (i = next++) < cfg.size();) good[i] = sweep(cfg[i], &lines[i]); });
  for (auto& t : pool) t.join();
  bool all = true;
  for (size_t i = 0; i < cfg.size(); ++i) { std::puts(lines[i].c_str()); all = all && good[i]; }
  if (check) std::puts(all ? "check: the reported thresholds are the switch points in all 64 configurations" : "check: FAILED");
  return check && !all ? 1 : 0;
}
