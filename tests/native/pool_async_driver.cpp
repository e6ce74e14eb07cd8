// Stand-alone driver for the render pool's begin / end pair (csrc/host_prep.cpp
// dmlp_host_pool_begin / dmlp_host_pool_end) and the step's prelude built on it.  Built plain and
// with -fsanitize=thread (tests/test_pool_async.py); the pool's size comes from
// DMLP_HOST_THREADS (workers = size - 1), so the test runs it once per size.
//   usage: pool_async_driver <expected pool size>
#include <atomic>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dmlp.h"

namespace {

int fails = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                          \
    }                                                                   \
  } while (0)

// Every part writes its own plain slot: a read of the slots after end is race-free only if end
// really waits for (and synchronises with) every worker — what TSan checks.
struct Job {
  long slot[32] = {0};
  int parts[32] = {0};
  std::atomic<int> calls{0};
};
void part_fn(void* c, int part, int parts) {
  Job& j = *(Job*)c;
  j.slot[part] += 1;
  j.parts[part] = parts;
  j.calls.fetch_add(1, std::memory_order_relaxed);
}

}  // namespace

int main(int argc, char** argv) {
  const int size = dmlp_host_threads();
  if (argc > 1) CHECK(size == std::atoi(argv[1]));
  const int workers = size - 1, parts = workers > 0 ? workers : 1;

  // end without begin
  CHECK(dmlp_host_pool_end() == -1);

  // back to back
  const int rounds = 10000;
  Job j;
  for (int i = 0; i < rounds; ++i) {
    CHECK(dmlp_host_pool_begin(part_fn, &j) == 0);
    CHECK(dmlp_host_pool_end() == 0);
  }
  CHECK(j.calls.load() == (long)rounds * parts);
  for (int p = 0; p < 32; ++p) {
    CHECK(j.slot[p] == (p < parts ? rounds : 0));
    CHECK(j.parts[p] == (p < parts ? parts : 0));
  }

  // the caller works between begin and end (its own data; then reads the workers')
  Job j2;
  std::vector<long> mine(1 << 12, 1);
  long sum = 0;
  for (int i = 0; i < 1000; ++i) {
    CHECK(dmlp_host_pool_begin(part_fn, &j2) == 0);
    for (long& v : mine) sum += v++;
    CHECK(dmlp_host_pool_end() == 0);
    long done = 0;
    for (int p = 0; p < parts; ++p) done += j2.slot[p];
    CHECK(done == (long)(i + 1) * parts);
  }
  CHECK(sum > 0);

  // inside an open pair: a second begin and a run are rejected and run nothing; a pass of the
  // library that wants the pool still returns a whole result (it runs on the caller)
  Job j3, j4;
  CHECK(dmlp_host_pool_begin(part_fn, &j3) == 0);
  CHECK(dmlp_host_pool_begin(part_fn, &j4) == -1);
  CHECK(dmlp_host_pool_run(part_fn, &j4) == -1);
  {
    std::vector<double> src(1 << 16);
    std::vector<int32_t> dst(src.size(), -1);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (double)((int)i - 30000) / 1.0e6;
    CHECK(dmlp_cpu_rows_i32(src.data(), (int64_t)src.size(), dst.data()) == 0);
    for (size_t i = 0; i < src.size(); ++i)
      if (dst[i] != (int)i - 30000) {
        CHECK(!"rows_i32 inside an open pair");
        break;
      }
    int lo = 0, hi = 0, x[4];
    CHECK(dmlp_host_prelude_begin(dst.data(), (int64_t)dst.size(), nullptr, 1, nullptr, 0, nullptr,
                                  nullptr, 0, 1, nullptr) == -1);
    CHECK(dmlp_host_prelude_end(&lo, &hi, x, x + 1) == -1);
  }
  CHECK(dmlp_host_pool_end() == 0);
  CHECK(j4.calls.load() == 0);
  CHECK(j3.calls.load() == parts);
  CHECK(dmlp_host_pool_end() == -1);
  CHECK(dmlp_host_pool_run(part_fn, &j4) == 0);  // the pool is whole again
  CHECK(j4.calls.load() == size);

  // the prelude on the pair, the caller busy meanwhile; a pool pass is rejected while it is open
  {
    const int64_t Q = 70001, N = 5000;
    const int A = 33;
    std::vector<int> k(Q), stage(Q, 0), lab(N);
    std::vector<double> X((size_t)N * A), mu(A), mu0(A);
    for (int64_t i = 0; i < Q; ++i) k[i] = 1 + (int)(i % 16);
    for (int64_t i = 0; i < N; ++i) lab[i] = (int)(i % 10) - 3;
    lab[N - 1] = INT_MAX;
    for (size_t i = 0; i < X.size(); ++i) X[i] = (double)(i % 1999) * 0.37 - 300.0;
    for (int it = 0; it < 200; ++it) {
      int k0 = 0, k1 = 0, l0 = 0, l1 = 0;
      CHECK(dmlp_host_prelude_begin(k.data(), Q, stage.data(), 1, lab.data(), 1, X.data(), nullptr,
                                    N, A, mu.data()) == 0);
      for (long& v : mine) sum += v++;
      if (it == 0) CHECK(dmlp_host_pool_run(part_fn, &j4) == -1);
      CHECK(dmlp_host_prelude_end(&k0, &k1, &l0, &l1) == 0);
      CHECK(k0 == 1 && k1 == 16 && l0 == -3 && l1 == INT_MAX);
      CHECK(stage == k);
      if (it == 0) mu0 = mu;
      CHECK(mu == mu0);
      stage[it] = -1;
    }
  }

  if (fails) {
    std::printf("pool async driver: %d FAILED (pool of %d)\n", fails, size);
    return 1;
  }
  std::printf("pool async driver: OK (pool of %d)\n", size);
  return 0;
}
