// engine_core.h — the distributed k-NN engine behind both front ends: the standalone
// `knn_engine` binary (engine_main.cpp) and the engine.h drop-in for the reference's own
// harness (dropin_engine.cpp).  KnnCore::KNN is Engine::KNN (engine.h:10-11): called on every
// rank, rank 0 holds the parsed input and receives the results.  Strategies (SURVEY.md
// §2.4 #16-21): farm (bench_4), shard_gather (bench_1), shard_reduce (bench_2/3), grid2d
// (engine.cpp), serial (bench.debug).  Data plane: RCCL over xGMI; control: MPI.
#pragma once
#include <unistd.h>

#include <chrono>
#include <climits>
#include <cstring>
#include <thread>

#include "engine_runtime.h"

namespace dmlp_rt {

// Page-locked host buffers (arena-backed) once a GPU runtime is up; every HostBuf<T> shares it.
inline bool& host_bufs_pinned() {
  static bool v = false;
  return v;
}

// Host array that is page-locked when a GPU is in use (H2D/D2H then run as DMA at full PCIe
// rate instead of through the runtime's pageable staging buffers).
template <typename T>
struct HostBuf {
  T* p = nullptr;
  size_t n = 0;
  bool pinned = false;
  // one switch for every element type (a per-T static left the drop-in's byte / int staging
  // pageable: synchronous staged copies)
  static bool& use_pinned() { return host_bufs_pinned(); }
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  HostBuf(HostBuf&& o) noexcept : p(o.p), n(o.n), pinned(o.pinned) { o.p = nullptr; o.n = 0; }
  HostBuf& operator=(HostBuf&& o) noexcept {
    std::swap(p, o.p); std::swap(n, o.n); std::swap(pinned, o.pinned);
    return *this;
  }
  void resize(size_t m) {
    release();
    n = m;
    if (!m) return;
    pinned = false;
    if (use_pinned()) {  // the library's page-locked arena, else hipHostMalloc
      p = (T*)dmlp_host_alloc((int64_t)(m * sizeof(T)));
      pinned = p != nullptr;
    }
    if (!pinned) p = (T*)std::malloc(m * sizeof(T));
    if (!p) throw std::runtime_error("host allocation failed");
  }
  void release() {
    if (p) { if (pinned) dmlp_host_free(p); else std::free(p); }
    p = nullptr; n = 0;
  }
  ~HostBuf() { release(); }
  T* data() { return p; }
  const T* data() const { return p; }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
};

struct Input {  // rank 0 only
  int64_t N = 0, Q = 0;
  int A = 0;
  std::vector<int> labels, k;
  HostBuf<double> X, Qx;
};

// where a one-rank call can stream its report (KnnCore::KNN_rows)
typedef void (*Sink)(void* ctx, const char* bytes, size_t n);

struct Output {  // rank 0 only
  std::vector<int> label;
  std::vector<uint64_t> cs;
  std::vector<double> dist;  // debug
  std::vector<int> ids;      // debug
  int kstride = 0;
  std::string report;        // host-rendered report (serial / debug)
  HostBuf<char> text;        // GPU-rendered report bytes (page-locked D2H target)
  size_t text_len = 0;
  const char* shared_text = nullptr;  // node-shared ingress: the report sits in the segment
};

// Node-shared ingress (KNN_INGRESS=shm, farm, P > 1 on one node): rank 0's parsed input copied
// once, before the timed region, into an MPI-3 shared-memory window that every rank maps and
// page-locks, plus an output region for the report (48 bytes per query bound).  Every rank then
// copies its own query block and the dataset over its OWN PCIe link (no funnel through GPU 0)
// and writes its report lines straight into the output region.
struct SharedIn {
  bool valid = false;
  int64_t N = 0, Q = 0;
  int A = 0;
  const double* X = nullptr;
  const int* labels = nullptr;
  const double* Qx = nullptr;
  const int* k = nullptr;
  char* out = nullptr;
  int64_t out_bytes = 0;
  void* plane = nullptr;  // the node render plane's region (dmlp_plane_bytes(N, A, 0)), or null
  int64_t plane_bytes = 0;
};

inline std::vector<char> read_all(const char* path) {
  FILE* f = (path && std::strcmp(path, "-") != 0) ? std::fopen(path, "rb") : stdin;
  if (!f) throw std::runtime_error("cannot open input");
  std::vector<char> buf;
  char tmp[1 << 16];
  size_t n;
  while ((n = std::fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
  if (f != stdin) std::fclose(f);
  return buf;
}

inline Input parse(const std::vector<char>& buf) {
  Input in;
  int64_t body = 0;
  if (dmlp_parse_header(buf.data(), (int64_t)buf.size(), &in.N, &in.Q, &in.A, &body) != 0)
    throw std::runtime_error("malformed header line");
  in.labels.resize(in.N);
  in.k.resize(in.Q);
  in.X.resize((size_t)in.N * in.A);
  in.Qx.resize((size_t)in.Q * in.A);
  const int64_t rc = dmlp_parse_body(buf.data(), (int64_t)buf.size(), body, in.N, in.Q, in.A,
                                     in.labels.data(), in.X.data(), in.k.data(), in.Qx.data(), 0);
  if (rc != 0)
    throw std::runtime_error("Line is wrongly formatted (line " + std::to_string(-rc + 1) + ")");
  return in;
}

class KnnCore {
 public:
  // warm_step: warm the native step up even at P > 1 (the drop-in's node-window farm)
  KnnCore(Runtime& rt, std::string strategy, bool debug, bool exact, bool dynamic = false,
          bool warm_step = false)
      : rt_(rt), strategy_(std::move(strategy)), debug_(debug), exact_(exact), dynamic_(dynamic),
        warm_step_(warm_step) {
    total_h_.resize(1);
    trace.init(rt_.rank, rt_.gpu ? rt_.stream : nullptr);
    if (strategy_ != "farm" && strategy_ != "shard_gather" && strategy_ != "shard_reduce" &&
        strategy_ != "serial" && strategy_ != "grid2d" && strategy_ != "ring")
      throw std::runtime_error("unknown strategy " + strategy_);
    if (dynamic_ && (strategy_ != "farm" || debug_))
      throw std::runtime_error("--schedule dynamic needs --strategy farm (and no --debug)");
    if (dynamic_) {
      // the chunk counter: one int64 in an MPI window on rank 0 (collective, untimed)
      MPI_Win_allocate(rt_.rank == 0 ? sizeof(int64_t) : 0, sizeof(int64_t), MPI_INFO_NULL,
                       MPI_COMM_WORLD, &ctr_base_, &ctr_win_);
    }
    if (rt_.gpu) warmup();
  }
  ~KnnCore() {
    if (ctr_win_ != MPI_WIN_NULL) MPI_Win_free(&ctr_win_);
    if (wake_st_) (void)hipStreamDestroy(wake_st_);
    if (ring_ev_) (void)hipEventDestroy(ring_ev_);
    if (ring_done_) (void)hipEventDestroy(ring_done_);
    if (ring_st_) (void)hipStreamDestroy(ring_st_);
    for (int b = 0; b < 2; ++b) {
      if (ooc_ready_[b]) (void)hipEventDestroy(ooc_ready_[b]);
      if (ooc_free_[b]) (void)hipEventDestroy(ooc_free_[b]);
    }
    if (ooc_st_) (void)hipStreamDestroy(ooc_st_);
  }

  // Engine::KNN — called on every rank; rank 0 holds `in` and receives `out`.
  // A 256 KiB device->host copy queued at the start of every call on a side stream: the D2H
  // copy path left idle since the untimed warm-up took ~7 ms to start the report's copy
  // (rocprofv3 timeline: a 6.9 ms gap between the formatter and a 10 us copy), while the
  // compute of the call hides this one.  KNN_WAKE_D2H=0 disables it (A/B).
  void wake_d2h() {
    if (!rt_.gpu || rt_.rank != 0 || !wake_) return;
    // the stream is created and used once in warmup(): the first operation on a new stream
    // pays ~18 ms of queue creation (tests/native/d2h_idle_probe.cpp)
    if (!wake_st_) HIPCHK(hipStreamCreateWithFlags(&wake_st_, hipStreamNonBlocking));
    const size_t n = size_t(256) << 10;
    if (wake_h_.size() < n) wake_h_.resize(n);
    HIPCHK(hipMemcpyAsync(wake_h_.data(), wscratch_.get(n), n, hipMemcpyDeviceToHost, wake_st_));
  }
  hipStream_t wake_st_ = nullptr;
  HostBuf<char> wake_h_;
  static constexpr int kMaxChunks = 16;
  double last_emit_ms = 0.0;  // the last KNN_rows' streamed report (0: none streamed)

  hipEvent_t emit_ev_[kMaxChunks] = {};
  // the device text of the last step -> out->text in `chunks` copies; sink gets each piece once
  // its copy completed (the host spins on the piece's event), in order
  void emit_chunks(int64_t len, int chunks, Output* out, Sink sink, void* sink_ctx) {
    out->text_len = (size_t)std::max<int64_t>(len, 0);
    if (len <= 0) return;
    const char* dev = nullptr;
    int64_t have = 0;
    DMLPCHK(dmlp_step_text(&dev, &have));
    if (have < len) throw std::runtime_error("emit: the device report is shorter than reported");
    if (out->text.size() < (size_t)len) out->text.resize((size_t)len);
    const int64_t piece = (len + chunks - 1) / chunks;
    int n = 0;
    for (int64_t off = 0; off < len; off += piece, ++n) {
      if (!emit_ev_[n]) HIPCHK(hipEventCreateWithFlags(&emit_ev_[n], hipEventDisableTiming));
      HIPCHK(hipMemcpyAsync(out->text.data() + off, dev + off, (size_t)std::min(piece, len - off),
                            hipMemcpyDeviceToHost, rt_.stream));
      HIPCHK(hipEventRecord(emit_ev_[n], rt_.stream));
    }
    int c = 0;
    for (int64_t off = 0; off < len; off += piece, ++c) {
      hipError_t e;
      while ((e = hipEventQuery(emit_ev_[c])) == hipErrorNotReady) {
      }
      HIPCHK(e);
      sink(sink_ctx, out->text.data() + off, (size_t)std::min(piece, len - off));
    }
  }
  bool wake_ = !(getenv("KNN_WAKE_D2H") && std::string(getenv("KNN_WAKE_D2H")) == "0");
  bool step_events_ = false;

  void set_shared(const SharedIn& s) { sh_ = s; }

  // The single-GPU step straight from tables of row pointers (the engine.h drop-in: the
  // harness's per-point attribute vectors; `in` carries N, Q, A, labels and k, no rows).  Returns
  // false, with nothing done, on more ranks or another strategy: the caller then packs the rows
  // and calls KNN.
  // One rank's block of a node-window call (the engine.h drop-in at P > 1, dropin_engine.cpp):
  // the native step on this rank's queries, the dataset through the node render plane (plane
  // rank 0 renders it from the harness's vectors Xr; the other ranks pass Xr = null), the report
  // kept on the device for emit_block.  Returns the report's byte count.
  int64_t step_block(const double* const* Xr, int64_t N, int A, const int* labels, int lo, int hi,
                     int kmax, const double* Qx, const double* const* Qr, const int* k, int64_t nq,
                     int64_t qid_base, const dmlp_plane* plane) {
    N_ = N; A_ = A; lo_ = lo; hi_ = hi; kmax_ = std::max(1, kmax); Q_ = nq;
    Output o;
    const dmlp_step_args a = step_host(nullptr, Xr, labels, Qx, Qr, k, nq, qid_base, 2, &o, plane);
    return a.report_len;
  }
  // the last step_block's report bytes -> dst (page-locked / registered), synchronously
  void emit_block(char* dst, int64_t len) {
    if (len) DMLPCHK(dmlp_step_emit(dst, len, rt_.stream));
  }

  // sink (optional, not in lists mode): the report goes to sink(ctx, bytes, n) in pieces as they
  // land on the host — the text stays on the device after the step and crosses in KNN_EMIT_CHUNKS
  // (default 4) copies, each piece handed over while the next one copies (the drop-in writes
  // them to the harness's stdout: the report's D2H runs under the write instead of before it)
  bool KNN_rows(Input* in, const double* const* Xr, const double* const* Qr, Output* out,
                Sink sink = nullptr, void* sink_ctx = nullptr) {
    last_emit_ms = 0.0;
    if (rt_.world != 1 || strategy_ != "farm" || dynamic_ || !fast_ || !in) return false;
    if (in->Q > (1 << 30)) return false;
    wake_d2h();
    N_ = in->N; Q_ = in->Q; A_ = in->A;
    // the label range and the largest k: scanned by the step on its render pool (hi <= lo, kmax
    // 0), not here on one thread — except for the lists mode, which sizes its outputs by kmax
    lo_ = 0; hi_ = 0;
    kmax_ = 0;
    if (debug_) {
      lo_ = 0; hi_ = 1;
      if (N_) {
        lo_ = *std::min_element(in->labels.begin(), in->labels.end());
        const int lmax = *std::max_element(in->labels.begin(), in->labels.end());
        if (lmax < INT_MAX) hi_ = lmax + 1;
        else lo_ = hi_ = 0;  // no int holds lmax + 1: "not given", every vote counts
      }
      kmax_ = Q_ ? std::max(1, *std::max_element(in->k.begin(), in->k.end())) : 1;
    }
    const int chunks = getenv("KNN_EMIT_CHUNKS") ? std::atoi(getenv("KNN_EMIT_CHUNKS")) : 4;
    if (sink && !debug_ && chunks > 1 && rt_.gpu) {
      const dmlp_step_args a = step_host(nullptr, Xr, in->labels.data(), nullptr, Qr,
                                         in->k.data(), Q_, 0, 2, out);
      trace.mark("report");
      const auto e0 = std::chrono::steady_clock::now();
      emit_chunks(a.report_len, std::min(chunks, kMaxChunks), out, sink, sink_ctx);
      last_emit_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - e0)
                         .count();
      trace.mark("emit_chunks");
      return true;
    }
    farm_step(in, Xr, Qr, out);
    trace.mark("report");
    return true;
  }

  void KNN(Input* in, Output* out) {
    wake_d2h();
    // sizes (engine.cpp:27-35): N, Q, A, label range, kmax
    int64_t meta[6] = {0, 0, 0, 0, 1, 1};
    if (rt_.rank == 0) {
      meta[0] = in->N;
      meta[1] = in->Q;
      meta[2] = in->A;
      if (in->N) {
        meta[3] = *std::min_element(in->labels.begin(), in->labels.end());
        meta[4] = (int64_t)*std::max_element(in->labels.begin(), in->labels.end()) + 1;
      }
      meta[5] = in->Q ? std::max(1, *std::max_element(in->k.begin(), in->k.end())) : 1;
    }
    MPI_Bcast(meta, 6, MPI_INT64_T, 0, MPI_COMM_WORLD);
    N_ = meta[0]; Q_ = meta[1]; A_ = (int)meta[2];
    lo_ = (int)meta[3]; hi_ = (int)meta[4]; kmax_ = (int)meta[5];
    if (strategy_ == "serial") return serial(in, out);
    if (strategy_ == "farm") return dynamic_ ? farm_dynamic(in, out) : farm(in, out);
    if (strategy_ == "grid2d") return grid2d(in, out);
    if (strategy_ == "ring") return ring(in, out);
    return sharded(in, out, strategy_ == "shard_reduce");
  }

 private:
  Runtime& rt_;
  std::string strategy_;
  bool debug_, exact_, dynamic_, warm_step_;
  // KNN_FAST=0 disables the single-GPU host-operand pipeline (A/B against the device path)
  bool fast_ = !(getenv("KNN_FAST") && std::string(getenv("KNN_FAST")) == "0");
  // host render + H2D of the screen operands in pipelined slices (the Python default too)
  MPI_Win ctr_win_ = MPI_WIN_NULL;
  int64_t* ctr_base_ = nullptr;
  DevBuf<int64_t> res_;
  int64_t N_ = 0, Q_ = 0;
  int A_ = 0, lo_ = 0, hi_ = 1, kmax_ = 1;
  DevBuf<double> X_, Qx_, d_, dall_, stage_d_;
  DevBuf<int> lab_, ids_, iall_, stage_i_, labout_, kd_;
  DevBuf<uint64_t> cs_;
  DevBuf<int64_t> off_;
  DevBuf<char> txt_, wscratch_;
  HostBuf<int64_t> total_h_;

 public:
  Trace trace;
  int64_t sent_ = 0;  // bytes this rank put on the wire (RCCL sends + its share of broadcasts)

 private:
  template <typename T>
  static ncclDataType_t nty();
  // Data plane.  RCCL over xGMI; with KNN_DATA_PLANE=host (Runtime::host_plane, a test mode
  // that lets several ranks share one GPU, which RCCL refuses) every transfer is staged through
  // host memory and carried by blocking MPI point-to-point calls in the same order, so the
  // strategies' offsets, trees and merge kernels run unchanged on the real kernels.  Every
  // point-to-point transfer is also logged (peer, bytes) for the KNN_P2P_CHECK matching check.
  void grp_start() {
    if (!rt_.host_plane) NCCLCHK(ncclGroupStart());
  }
  void grp_end() {
    if (!rt_.host_plane) NCCLCHK(ncclGroupEnd());
  }
  // (st: the stream the transfer is ordered on; default the engine stream)
  template <typename T>
  void snd(const T* p, int64_t n, int peer, hipStream_t st = nullptr) {
    if (!st) st = rt_.stream;
    const int64_t bytes = n * (int64_t)sizeof(T);
    p2p_log_.push_back({1, peer, bytes});
    sent_ += bytes;
    if (!rt_.host_plane) {
      NCCLCHK(ncclSend(p, n, nty<T>(), peer, rt_.nccl, st));
      return;
    }
    std::vector<char> h(bytes);
    HIPCHK(hipMemcpyAsync(h.data(), p, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    mpi_bytes(h.data(), bytes, peer, true);
  }
  template <typename T>
  void rcv(T* p, int64_t n, int peer, hipStream_t st = nullptr) {
    if (!st) st = rt_.stream;
    const int64_t bytes = n * (int64_t)sizeof(T);
    p2p_log_.push_back({0, peer, bytes});
    if (!rt_.host_plane) {
      NCCLCHK(ncclRecv(p, n, nty<T>(), peer, rt_.nccl, st));
      return;
    }
    std::vector<char> h(bytes);
    mpi_bytes(h.data(), bytes, peer, false);
    HIPCHK(hipMemcpyAsync(p, h.data(), bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // h dies here
  }
  // One ring exchange: send `cur` to the next rank, receive the previous rank's into `nxt`.  In
  // host-staged mode the blocking MPI pair is ordered by rank parity so it cannot deadlock.
  template <typename T>
  void ring_exchange(const T* cur, T* nxt, int64_t n, hipStream_t st) {
    const int P = rt_.world, r = rt_.rank;
    const int to = (r + 1) % P, from = (r + P - 1) % P;
    if (!rt_.host_plane) {
      grp_start();
      snd(cur, n, to, st);
      rcv(nxt, n, from, st);
      grp_end();
      return;
    }
    if (r % 2 == 0) { snd(cur, n, to, st); rcv(nxt, n, from, st); }
    else { rcv(nxt, n, from, st); snd(cur, n, to, st); }
  }
  // Equal-size all-gather of `bytes` per rank from `chunk` into `full` (rank order), on the engine
  // stream: one ncclAllGather over xGMI, or host-staged MPI_Allgather in the test data plane.
  void allgather_bytes(const void* chunk, void* full, int64_t bytes) {
    sent_ += bytes * (rt_.world - 1);
    if (!rt_.host_plane) {
      NCCLCHK(ncclAllGather(chunk, full, (size_t)bytes, ncclUint8, rt_.nccl, rt_.stream));
      return;
    }
    if (bytes > (int64_t)INT32_MAX / rt_.world) throw std::runtime_error("all-gather too large");
    std::vector<char> h(bytes), all(bytes * rt_.world);
    HIPCHK(hipMemcpyAsync(h.data(), chunk, bytes, hipMemcpyDeviceToHost, rt_.stream));
    rt_.sync();
    MPI_Allgather(h.data(), (int)bytes, MPI_BYTE, all.data(), (int)bytes, MPI_BYTE, MPI_COMM_WORLD);
    HIPCHK(hipMemcpyAsync(full, all.data(), bytes * rt_.world, hipMemcpyHostToDevice, rt_.stream));
    rt_.sync();  // `all` dies here
  }
  template <typename T>
  void bcast(T* p, int64_t n) {
    const int64_t bytes = n * (int64_t)sizeof(T);
    if (rt_.rank == 0) sent_ += bytes * (rt_.world - 1);
    if (!rt_.host_plane) {
      NCCLCHK(ncclBroadcast(p, p, n, nty<T>(), 0, rt_.nccl, rt_.stream));
      return;
    }
    std::vector<char> h(bytes);
    if (rt_.rank == 0) {
      HIPCHK(hipMemcpyAsync(h.data(), p, bytes, hipMemcpyDeviceToHost, rt_.stream));
      rt_.sync();
    }
    for (int64_t o = 0; o < bytes; o += kMpiChunk)
      MPI_Bcast(h.data() + o, (int)std::min<int64_t>(kMpiChunk, bytes - o), MPI_BYTE, 0,
                MPI_COMM_WORLD);
    if (rt_.rank != 0) {
      HIPCHK(hipMemcpyAsync(p, h.data(), bytes, hipMemcpyHostToDevice, rt_.stream));
      rt_.sync();
    }
  }
  static constexpr int64_t kMpiChunk = int64_t(1) << 30;
  static void mpi_bytes(char* p, int64_t bytes, int peer, bool send) {
    for (int64_t o = 0; o < bytes; o += kMpiChunk) {
      const int c = (int)std::min<int64_t>(kMpiChunk, bytes - o);
      if (send) MPI_Send(p + o, c, MPI_BYTE, peer, 77, MPI_COMM_WORLD);
      else MPI_Recv(p + o, c, MPI_BYTE, peer, 77, MPI_COMM_WORLD, MPI_STATUS_IGNORE);
    }
  }

 public:
  struct P2PEntry {
    int64_t send, peer, bytes;
  };
  std::vector<P2PEntry> p2p_log_;
  // KNN_P2P_CHECK: every rank's ordered (send/recv, peer, bytes) log goes to rank 0, which checks
  // that the sends from a to b and the receives at b from a are the same sequence of sizes (a
  // mismatched ncclSend/ncclRecv pair hangs or corrupts; this catches it on any host, even
  // with the host-staged plane).  Returns the number of matched messages; throws on mismatch.
  int64_t check_p2p() {
    const int P = rt_.world;
    std::vector<int64_t> flat;
    for (const auto& e : p2p_log_) { flat.push_back(e.send); flat.push_back(e.peer); flat.push_back(e.bytes); }
    int n = (int)flat.size();
    std::vector<int> counts(P), displs(P);
    MPI_Gather(&n, 1, MPI_INT, counts.data(), 1, MPI_INT, 0, MPI_COMM_WORLD);
    std::vector<int64_t> all;
    if (rt_.rank == 0) {
      int tot = 0;
      for (int r = 0; r < P; ++r) { displs[r] = tot; tot += counts[r]; }
      all.resize(std::max(1, tot));
    }
    MPI_Gatherv(flat.data(), n, MPI_INT64_T, all.data(), counts.data(), displs.data(),
                MPI_INT64_T, 0, MPI_COMM_WORLD);
    int64_t matched = 0;
    if (rt_.rank == 0) {
      // seq[a][b] = sizes a sent to b; got[b][a] = sizes b received from a
      std::vector<std::vector<std::vector<int64_t>>> seq(P, std::vector<std::vector<int64_t>>(P)),
          got(P, std::vector<std::vector<int64_t>>(P));
      for (int r = 0; r < P; ++r)
        for (int i = 0; i < counts[r]; i += 3) {
          const int64_t* e = all.data() + displs[r] + i;
          if (e[1] < 0 || e[1] >= P) throw std::runtime_error("p2p check: bad peer");
          (e[0] ? seq[r][e[1]] : got[r][e[1]]).push_back(e[2]);
        }
      for (int a = 0; a < P; ++a)
        for (int b = 0; b < P; ++b) {
          if (seq[a][b] != got[b][a])
            throw std::runtime_error("p2p check: rank " + std::to_string(a) + " -> " +
                                     std::to_string(b) + ": " + std::to_string(seq[a][b].size()) +
                                     " sends vs " + std::to_string(got[b][a].size()) +
                                     " receives (or sizes differ)");
          matched += (int64_t)seq[a][b].size();
        }
    }
    p2p_log_.clear();
    return matched;
  }

 private:

  void warmup() {
    // the RCCL group wrappers run here once, on every run: an empty ncclGroupStart/End pair is
    // valid at any world size, so a single-GPU test exercises the code the multi-GPU path uses
    grp_start();
    grp_end();
    (void)dmlp_host_threads();  // the host conversion pool's threads start here, untimed
    wake_d2h();                 // creates its stream and runs its first copy, untimed
    if (wake_st_) HIPCHK(hipStreamSynchronize(wake_st_));
    // load every kernel once (module load + first-launch costs stay outside the timed region)
    const int n = 256, q = 64, a = 8;
    std::vector<double> x(n * a), qq(q * a);
    std::vector<int> lab(n), k(q);
    for (int i = 0; i < n * a; ++i) x[i] = (i * 37 % 101) * 0.5;
    for (int i = 0; i < q * a; ++i) qq[i] = (i * 53 % 97) * 0.5;
    for (int i = 0; i < n; ++i) lab[i] = i % 3;
    for (int i = 0; i < q; ++i) k[i] = 1 + (i * 7) % 60;
    double* xd = X_.get(n * a);
    double* qd = Qx_.get(q * a);
    int* ld = lab_.get(n);
    HIPCHK(hipMemcpy(xd, x.data(), x.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(qd, qq.data(), qq.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ld, lab.data(), lab.size() * 4, hipMemcpyHostToDevice));
    A_ = a;
    DMLPCHK(dmlp_knn_local(xd, n, a, qd, q, k.data(), 64, d_.get(q * 64), ids_.get(q * 64), ld, 0,
                           3, labout_.get(q), cs_.get(q), exact_ ? 1 : 0, rt_.stream));
    int64_t* off = off_.get(dmlp_format_scratch(q));
    DMLPCHK(dmlp_format_report(cs_.p, q, 0, off, txt_.get(dmlp_format_bound(q)), rt_.stream));
    rt_.sync();
    // The first large async copy in each direction pays a one-time ~6-8 ms runtime setup
    // (measured: tests/native/h2d_probe.cpp) — and the KNN call is the first copy otherwise.
    // Run synchronised H2D and D2H copies of several sizes through pinned staging (and a
    // pageable H2D) here, untimed: each copy path initialises on its first use.
    {
      const size_t wb = size_t(32) << 20;
      HostBuf<char> hb;
      hb.resize(wb);
      std::memset(hb.data(), 0, wb);
      char* db = wscratch_.get(wb);
      for (size_t sz = size_t(64) << 10; sz <= wb; sz *= 8) {
        HIPCHK(hipMemcpyAsync(db, hb.data(), sz, hipMemcpyHostToDevice, rt_.stream));
        rt_.sync();
        HIPCHK(hipMemcpyAsync(hb.data(), db, sz, hipMemcpyDeviceToHost, rt_.stream));
        rt_.sync();
      }
      std::vector<char> pg(wb / 8, 1);
      HIPCHK(hipMemcpyAsync(db, pg.data(), pg.size(), hipMemcpyHostToDevice, rt_.stream));
      HIPCHK(hipMemcpyAsync(pg.data(), db, pg.size(), hipMemcpyDeviceToHost, rt_.stream));
      rt_.sync();
    }
    const bool shm_ingress = getenv("KNN_INGRESS") && std::string(getenv("KNN_INGRESS")) == "shm";
    if ((rt_.world == 1 || shm_ingress || warm_step_) && fast_) {
      // the native step once on a tiny input, every k class (early start at k <= 32, the
      // two-pass screen above): its side stream, events, staging and device buffers, the host
      // pool's first job and the first copies on the side stream are all paid here (measured
      // ~16 ms of first-use cost otherwise)
      Input w;
      w.N = 300; w.Q = 70; w.A = 8;
      w.labels.resize(w.N);
      w.k.resize(w.Q);
      w.X.resize(w.N * w.A);
      w.Qx.resize(w.Q * w.A);
      for (int64_t i = 0; i < w.N * w.A; ++i) w.X.data()[i] = (double)((i * 37) % 101);
      for (int64_t i = 0; i < w.Q * w.A; ++i) w.Qx.data()[i] = (double)((i * 53) % 97);
      for (int64_t i = 0; i < w.N; ++i) w.labels[i] = (int)(i % 3);
      for (int64_t i = 0; i < w.Q; ++i) w.k[i] = 1 + (int)(i % 32);
      N_ = w.N; Q_ = w.Q; A_ = w.A; lo_ = 0; hi_ = 3;
      for (int pass = 0; pass < 2; ++pass) {
        for (int64_t i = 0; i < w.Q; ++i) w.k[i] = 1 + (int)(i % (pass ? 60 : 32));
        kmax_ = pass ? 60 : 32;
        Output o;
        (void)step_host(w.X.data(), nullptr, w.labels.data(), w.Qx.data(), nullptr, w.k.data(),
                        w.Q, 0, rt_.world == 1 ? 1 : 2, &o);
      }
      step_calls_ = 0;
      rt_.sync();
    }
    MPI_Barrier(MPI_COMM_WORLD);
  }

  void local_knn(const double* Xd, int64_t n, const double* Qd, int64_t nq, const int* kh,
                 double* od, int* oi, const int* labels, int* lab, uint64_t* cs) {
    // the library's one dispatcher (pipeline.hip): per-query classes, escalation, exact paths
    DMLPCHK(dmlp_knn_local(Xd, n, A_, Qd, nq, kh, kmax_, od, oi, labels, lo_, hi_, lab, cs,
                           exact_ ? 1 : 0, rt_.stream));
  }

  // rank 0: the report (GPU formatter) or, with --debug, the host copies of the lists + labels
  void render(Output* out, const uint64_t* cs_dev, const int* lab_dev, const double* dd,
              const int* ii) {
    out->kstride = kmax_;
    if (!debug_) {
      int64_t* off = off_.get(dmlp_format_scratch((int)Q_));
      const size_t bound = (size_t)dmlp_format_bound((int)Q_);
      if (out->text.size() < bound) out->text.resize(bound);
      // Render on the device, then ONE copy of the bound-sized text into the page-locked output
      // (no wait for the byte count first).  Formatter stores straight into host memory over
      // the link measured ~7 ms for 6 MB; the copy engine moves it in ~0.12 ms (the arena's
      // pages were DMA-mapped at reservation, so the first copy pays no mapping cost).
      char* txt = txt_.get(bound);
      DMLPCHK(dmlp_format_report(cs_dev, (int)Q_, 0, off, txt, rt_.stream));
      trace.mark("format");
      int64_t* total = total_h_.data();
      HIPCHK(hipMemcpyAsync(total, off + Q_, 8, hipMemcpyDeviceToHost, rt_.stream));
      HIPCHK(hipMemcpyAsync(out->text.data(), txt, bound, hipMemcpyDeviceToHost, rt_.stream));
      rt_.sync();
      out->text_len = *total;
      return;
    }
    rt_.sync();
    out->label.resize(Q_);
    out->dist.resize(Q_ * kmax_);
    out->ids.resize(Q_ * kmax_);
    HIPCHK(hipMemcpy(out->label.data(), lab_dev, Q_ * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out->dist.data(), dd, Q_ * kmax_ * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out->ids.data(), ii, Q_ * kmax_ * 4, hipMemcpyDeviceToHost));
    out->report.clear();
  }

  // ---------------------------------------------------------------- the native step
  // Every single-GPU call from host rows goes through the library's one pipeline (pipeline.hip
  // dmlp_step, also behind the Python engine): host render of the screen operands, early start,
  // fp64 rows behind the screen, exact re-rank, vote, checksum, report text on the GPU, per-query
  // escalation.  Xr / Qr (non-null): tables of row pointers (the engine.h drop-in reads the
  // harness's per-point vectors in place); else X / Qx row-major.  report_mode 1: the text into
  // out->text (page-locked); 2: kept on the device for a multi-rank egress (dmlp_step_emit);
  // lists mode (debug_): the sorted lists + labels into dd / ii / lb instead.
  DevBuf<double> sd_;
  DevBuf<int> si_, slb_;
  DevBuf<uint64_t> scs_;
  int64_t step_calls_ = 0;

 public:
  int64_t step_calls() const { return step_calls_; }
  dmlp_step_args last_step_{};

 private:
  dmlp_step_args step_host(const double* X, const double* const* Xr, const int* labels,
                           const double* Qx, const double* const* Qr, const int* k, int64_t nq,
                           int64_t qid_base, int report_mode, Output* out,
                           const dmlp_plane* plane = nullptr) {
    dmlp_step_args a{};
    a.plane = plane;
    a.X = X; a.Xr = Xr; a.N = N_; a.A = A_;
    a.labels = labels; a.label_lo = lo_; a.label_hi = hi_;
    a.Qx = Qx; a.Qr = Qr; a.k = k; a.Q = nq;
    a.kmin = 1; a.kmax = 0;  // scanned by the step (this rank's own block)
    a.qid_base = qid_base;
    a.exact = exact_ ? 1 : 0;
    const int64_t qs = std::max<int64_t>(nq, 1);
    a.out_lab = slb_.get(qs);
    a.out_cs = scs_.get(qs);
    a.kstride = kmax_;
    if (debug_) {
      a.out_d = sd_.get(qs * kmax_);
      a.out_i = si_.get(qs * kmax_);
    }
    a.report_mode = debug_ ? 0 : report_mode;
    if (a.report_mode == 1) {
      const size_t bound = (size_t)dmlp_format_bound((int)nq);
      if (out->text.size() < bound) out->text.resize(bound);
      a.report_dst = out->text.data();
      a.report_cap = (int64_t)out->text.size();
    }
    a.stream = rt_.stream;
    if (trace.on && !step_events_) step_events_ = dmlp_step_events(1) == 0;
    trace.mark("step_enter");
    DMLPCHK(dmlp_step(&a));
    ++step_calls_;
    last_step_ = a;
    trace.mark("step");
    if (trace.on) {
      int64_t st[8];
      dmlp_pipeline_stats(st);
      std::fprintf(stderr, "[dmlp-step] rank %d path %d early %d escalated %d exact %lld "
                   "early_waits %d early_timeouts %d\n", rt_.rank, a.path, a.early,
                   a.n_escalated, (long long)st[0], a.early_waits, a.early_timeouts);
      // KNN_TRACE: the step's own hipEvent timeline (ms from step entry)
      double ms[16];
      const char* nm[16];
      const int n = dmlp_step_timeline(ms, nm, 16);
      std::fprintf(stderr, "[dmlp-step] rank %d timeline", rt_.rank);
      for (int i = 0; i < n; ++i) std::fprintf(stderr, " %s %.3f", nm[i], ms[i]);
      std::fprintf(stderr, "\n");
    }
    return a;
  }

  // one rank holds everything: the whole call is one step
  void farm_step(Input* in, const double* const* Xr, const double* const* Qr, Output* out) {
    const dmlp_step_args a = step_host(Xr ? nullptr : in->X.data(), Xr, in->labels.data(),
                                       Qr ? nullptr : in->Qx.data(), Qr, in->k.data(), Q_, 0, 1,
                                       out);
    out->kstride = kmax_;
    if (!debug_) {
      out->text_len = (size_t)a.report_len;
      return;
    }
    out->label.resize(Q_);
    out->dist.resize(Q_ * kmax_);
    out->ids.resize(Q_ * kmax_);
    HIPCHK(hipMemcpy(out->label.data(), a.out_lab, Q_ * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out->dist.data(), a.out_d, Q_ * kmax_ * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out->ids.data(), a.out_i, Q_ * kmax_ * 4, hipMemcpyDeviceToHost));
    out->report.clear();
  }

  // Farm over the node-shared segment, P > 1: every rank runs the step on its own query block
  // straight from the segment (its own PCIe link), keeps its report lines on its GPU, and copies
  // them into the segment's output region at its byte offset once the lengths are known (one
  // MPI_Allgather of 8 bytes); a barrier, and rank 0 holds the whole report.
  bool farm_step_shared(Output* out) {
    const int P = rt_.world, r = rt_.rank;
    if (debug_ || sh_.N != N_ || sh_.Q != Q_ || sh_.A != A_) return false;
    std::vector<int64_t> cnt, off;
    block_partition(Q_, P, cnt, off);
    const int64_t a0 = off[r], nl = cnt[r];
    int64_t len = 0;
    // the replicated dataset's image and rows rendered once for the node, 1/P by each rank, into
    // the window's render plane (KNN_PLANE=0: every rank renders all of it)
    dmlp_plane pl{};
    const bool use_plane = sh_.plane && P > 1 && plane_on_;
    if (use_plane) {
      pl.base = sh_.plane;
      pl.bytes = sh_.plane_bytes;
      pl.rank = r;
      pl.renderers = P;
      pl.gen = ++plane_gen_;
    }
    // (a rank without queries still renders its share of the plane)
    if (nl || use_plane) {
      const dmlp_step_args a = step_host(sh_.X, nullptr, sh_.labels, sh_.Qx + a0 * A_, nullptr,
                                         sh_.k + a0, nl, a0, 2, out, use_plane ? &pl : nullptr);
      len = a.report_len;
    }
    std::vector<int64_t> lens(P);
    MPI_Allgather(&len, 1, MPI_INT64_T, lens.data(), 1, MPI_INT64_T, MPI_COMM_WORLD);
    int64_t at = 0, total = 0;
    for (int i = 0; i < P; ++i) {
      if (i < r) at += lens[i];
      total += lens[i];
    }
    if (total > sh_.out_bytes) throw std::runtime_error("shared output region too small");
    if (len) DMLPCHK(dmlp_step_emit(sh_.out + at, len, rt_.stream));
    MPI_Barrier(MPI_COMM_WORLD);  // every block is in the segment
    if (r == 0) {
      out->kstride = kmax_;
      out->shared_text = sh_.out;
      out->text_len = (size_t)total;
    }
    trace.mark("report");
    return true;
  }
  SharedIn sh_;
  int64_t plane_gen_ = 0;
  bool plane_on_ = !(getenv("KNN_PLANE") && std::string(getenv("KNN_PLANE")) == "0");

  // ---------------------------------------------------------------- farm (bench_4)
  // ---------------------------------------------------------------- out-of-core farm
  // KNN_MAX_DEVICE_ROWS=R with N > R (SURVEY.md §5 "datasets beyond HBM"; Python twin:
  // ops/knn.py knn_gpu_streamed): the dataset never sits whole on a GPU.  Rank 0 streams it
  // from host memory in R-row chunks, double-buffered — the H2D of chunk c + 1 runs on a side
  // stream while chunk c is screened and re-ranked — each chunk is broadcast to the other ranks,
  // every rank screens its query block against it and merges the chunk's lists into its
  // running top-k (K-way merge kernel); labels, vote and checksum once at the end.
  int64_t ooc_rows_ = getenv("KNN_MAX_DEVICE_ROWS") ? std::atoll(getenv("KNN_MAX_DEVICE_ROWS")) : 0;
  DevBuf<double> ooc_buf_[2];
  hipStream_t ooc_st_ = nullptr;
  hipEvent_t ooc_ready_[2] = {nullptr, nullptr}, ooc_free_[2] = {nullptr, nullptr};
  void farm_ooc(Input* in, Output* out) {
    const int P = rt_.world, r = rt_.rank;
    hipStream_t st = rt_.stream;
    if (!ooc_st_) {
      HIPCHK(hipStreamCreateWithFlags(&ooc_st_, hipStreamNonBlocking));
      for (int b = 0; b < 2; ++b) {
        HIPCHK(hipEventCreateWithFlags(&ooc_ready_[b], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ooc_free_[b], hipEventDisableTiming));
      }
    }
    std::vector<int64_t> cnt, off;
    block_partition(Q_, P, cnt, off);
    const int64_t nl = cnt[r];
    const int64_t R = ooc_rows_, nchunks = (N_ + R - 1) / R;
    int* Ld = lab_.get(N_);
    double* Qall = Qx_.get((r == 0 ? Q_ : nl) * A_ + 1);
    double* buf[2] = {ooc_buf_[0].get(R * A_), ooc_buf_[1].get(R * A_)};
    auto h2d_chunk = [&](int64_t c) {
      const int64_t a = c * R, n = std::min(R, N_ - a);
      const int b = (int)(c & 1);
      if (c >= 2) HIPCHK(hipStreamWaitEvent(ooc_st_, ooc_free_[b], 0));  // chunk c - 2 done
      HIPCHK(hipMemcpyAsync(buf[b], in->X.data() + a * A_, n * A_ * 8, hipMemcpyHostToDevice,
                            ooc_st_));
      HIPCHK(hipEventRecord(ooc_ready_[b], ooc_st_));
    };
    if (r == 0) {
      HIPCHK(hipMemcpyAsync(Ld, in->labels.data(), N_ * 4, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(Qall, in->Qx.data(), Q_ * A_ * 8, hipMemcpyHostToDevice, st));
      h2d_chunk(0);
    }
    std::vector<int> kl(std::max<int64_t>(1, nl)), sc(P), so(P);
    for (int t = 0; t < P; ++t) { sc[t] = (int)cnt[t]; so[t] = (int)off[t]; }
    MPI_Scatterv(r == 0 ? in->k.data() : nullptr, sc.data(), so.data(), MPI_INT, kl.data(), sc[r],
                 MPI_INT, 0, MPI_COMM_WORLD);
    if (P > 1) {
      bcast(Ld, N_);
      grp_start();
      if (r == 0) {
        for (int t = 1; t < P; ++t)
          if (cnt[t]) snd(Qall + off[t] * A_, cnt[t] * A_, t);
      } else if (nl) {
        rcv(Qall, nl * A_, 0);
      }
      grp_end();
    }
    trace.mark("distribute");
    const int64_t L = std::max<int64_t>(1, nl) * kmax_;
    double* sd = ring_d_.get(2 * L);  // [running | this chunk's] lists
    int* si = ring_i_.get(2 * L);
    double* dd = d_.get(std::max<int64_t>(L, r == 0 ? Q_ * kmax_ : 1));
    int* ii = ids_.get(std::max<int64_t>(L, r == 0 ? Q_ * kmax_ : 1));
    int* kd = kd_.get(std::max<int64_t>(1, nl));
    if (nl) HIPCHK(hipMemcpyAsync(kd, kl.data(), nl * 4, hipMemcpyHostToDevice, st));
    for (int64_t c = 0; c < nchunks; ++c) {
      const int64_t a = c * R, n = std::min(R, N_ - a);
      const int b = (int)(c & 1);
      if (r == 0) {
        if (c + 1 < nchunks) h2d_chunk(c + 1);  // the next chunk crosses PCIe meanwhile
        HIPCHK(hipStreamWaitEvent(st, ooc_ready_[b], 0));
      }
      if (P > 1) bcast(buf[b], n * A_);
      if (nl) {
        double* od = c ? sd + L : sd;
        int* oi = c ? si + L : si;
        local_knn(buf[b], n, Qall, nl, kl.data(), od, oi, nullptr, nullptr, nullptr);
        DMLPCHK(dmlp_offset_ids(oi, L, (int)a, st));
        if (c) {
          DMLPCHK(dmlp_merge(sd, si, 2, L, kmax_, kd, (int)nl, dd, ii, kmax_, st));
          HIPCHK(hipMemcpyAsync(sd, dd, L * 8, hipMemcpyDeviceToDevice, st));
          HIPCHK(hipMemcpyAsync(si, ii, L * 4, hipMemcpyDeviceToDevice, st));
        }
      }
      HIPCHK(hipEventRecord(ooc_free_[b], st));
    }
    trace.mark("compute");
    int* lb = labout_.get((r == 0 ? Q_ : nl) + 1);
    uint64_t* cs = cs_.get((r == 0 ? Q_ : nl) + 1);
    if (nl) DMLPCHK(dmlp_finalize(sd, si, kmax_, kd, nullptr, (int)nl, Ld, lo_, hi_, lb, cs, st));
    if (r == 0 && nl) {  // rank 0's own lists at the head of the gathered arrays
      HIPCHK(hipMemcpyAsync(dd, sd, nl * kmax_ * 8, hipMemcpyDeviceToDevice, st));
      HIPCHK(hipMemcpyAsync(ii, si, nl * kmax_ * 4, hipMemcpyDeviceToDevice, st));
    }
    if (P > 1) {
      grp_start();
      if (r == 0) {
        for (int t = 1; t < P; ++t) {
          if (!cnt[t]) continue;
          rcv(lb + off[t], cnt[t], t);
          rcv(cs + off[t], cnt[t], t);
          if (debug_) {
            rcv(dd + off[t] * kmax_, cnt[t] * kmax_, t);
            rcv(ii + off[t] * kmax_, cnt[t] * kmax_, t);
          }
        }
      } else if (nl) {
        snd(lb, nl, 0);
        snd(cs, nl, 0);
        if (debug_) {
          snd(sd, nl * kmax_, 0);
          snd(si, nl * kmax_, 0);
        }
      }
      grp_end();
    }
    trace.mark("gather");
    if (r == 0) render(out, cs, lb, dd, ii);
    trace.mark("report");
    rt_.sync();
  }

  void farm(Input* in, Output* out) {
    const int P = rt_.world;
    if (ooc_rows_ > 0 && N_ > ooc_rows_) return farm_ooc(in, out);
    if (P == 1 && fast_ && Q_ <= (1 << 30)) {
      farm_step(in, nullptr, nullptr, out);
      trace.mark("report");
      return;
    }
    if (P > 1 && sh_.valid && fast_ && farm_step_shared(out)) return;
    std::vector<int64_t> cnt, off;
    block_partition(Q_, P, cnt, off);
    double* Xd = X_.get(N_ * A_);
    int* Ld = lab_.get(N_);
    double* Qall = Qx_.get((rt_.rank == 0 ? Q_ : cnt[rt_.rank]) * A_ + 1);
    hipStream_t st = rt_.stream;
    if (rt_.rank == 0) {
      HIPCHK(hipMemcpyAsync(Xd, in->X.data(), N_ * A_ * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(Ld, in->labels.data(), N_ * 4, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(Qall, in->Qx.data(), Q_ * A_ * 8, hipMemcpyHostToDevice, st));
    }
    trace.mark("h2d");
    // per-rank k on the host (tiny, MPI) — it drives kernel dispatch
    std::vector<int> kl(cnt[rt_.rank]);
    std::vector<int> sc(P), so(P);
    for (int r = 0; r < P; ++r) { sc[r] = (int)cnt[r]; so[r] = (int)off[r]; }
    MPI_Scatterv(rt_.rank == 0 ? in->k.data() : nullptr, sc.data(), so.data(), MPI_INT,
                 kl.data(), sc[rt_.rank], MPI_INT, 0, MPI_COMM_WORLD);
    if (P > 1) {
      // replicate the dataset (MPI_Bcast of all rows in bench_4 -> ncclBroadcast over xGMI)
      bcast(Xd, N_ * A_);
      bcast(Ld, N_);
      // static query blocks: one direct xGMI hop per rank
      grp_start();
      if (rt_.rank == 0) {
        for (int r = 1; r < P; ++r)
          if (cnt[r]) snd(Qall + off[r] * A_, cnt[r] * A_, r);
      } else if (cnt[rt_.rank]) {
        rcv(Qall, cnt[rt_.rank] * A_, 0);
      }
      grp_end();
    }
    trace.mark("distribute");
    const int64_t nl = cnt[rt_.rank];
    double* dd = d_.get(std::max<int64_t>(1, (rt_.rank == 0 ? Q_ : nl)) * kmax_);
    int* ii = ids_.get(std::max<int64_t>(1, (rt_.rank == 0 ? Q_ : nl)) * kmax_);
    int* lb = labout_.get(rt_.rank == 0 ? Q_ : nl + 1);
    uint64_t* cs = cs_.get(rt_.rank == 0 ? Q_ : nl + 1);
    local_knn(Xd, N_, Qall, nl, kl.data(), dd, ii, Ld, lb, cs);
    trace.mark("compute");
    if (P > 1) {  // gather (label, checksum [, lists]) to rank 0 in rank order
      grp_start();
      if (rt_.rank == 0) {
        for (int r = 1; r < P; ++r) {
          if (!cnt[r]) continue;
          rcv(lb + off[r], cnt[r], r);
          rcv(cs + off[r], cnt[r], r);
          if (debug_) {
            rcv(dd + off[r] * kmax_, cnt[r] * kmax_, r);
            rcv(ii + off[r] * kmax_, cnt[r] * kmax_, r);
          }
        }
      } else if (nl) {
        snd(lb, nl, 0);
        snd(cs, nl, 0);
        if (debug_) {
          snd(dd, nl * kmax_, 0);
          snd(ii, nl * kmax_, 0);
        }
      }
      grp_end();
    }
    trace.mark("gather");
    if (rt_.rank == 0) render(out, cs, lb, dd, ii);
    trace.mark("report");
    rt_.sync();
  }

  // ---------------------------------------------------------------- dynamic farm (bench_4)
  // bench_4's master hands out work per query on request (@0xd80c Recv ANY_SOURCE -> @0xd986
  // Send).  Here no rank is a master: every rank holds the replicated dataset and all queries
  // (broadcast over xGMI), claims query chunks with an MPI-3 atomic fetch-and-add on a counter
  // in rank 0's window (passive target, no progress thread on rank 0 needed), writes each
  // chunk's (label, checksum) into its own zero-initialised full-length arrays, and one sum
  // reduce (each element non-zero on exactly one rank) lands every result on rank 0.
  int64_t claim() {
    const int64_t one = 1;
    int64_t got = 0;
    MPI_Win_lock(MPI_LOCK_SHARED, 0, 0, ctr_win_);
    MPI_Fetch_and_op(&one, &got, MPI_INT64_T, 0, 0, MPI_SUM, ctr_win_);
    MPI_Win_unlock(0, ctr_win_);
    return got;
  }
  template <typename T>
  void reduce_sum_to_root(T* p, int64_t n, MPI_Datatype mt, ncclDataType_t nt) {
    if (!rt_.host_plane) {
      NCCLCHK(ncclReduce(p, p, n, nt, ncclSum, 0, rt_.nccl, rt_.stream));
      return;
    }
    std::vector<T> h(n), r(rt_.rank == 0 ? n : 0);
    HIPCHK(hipMemcpyAsync(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost, rt_.stream));
    rt_.sync();
    MPI_Reduce(h.data(), r.data(), (int)n, mt, MPI_SUM, 0, MPI_COMM_WORLD);
    if (rt_.rank == 0) {
      HIPCHK(hipMemcpyAsync(p, r.data(), n * sizeof(T), hipMemcpyHostToDevice, rt_.stream));
      rt_.sync();
    }
  }
  void farm_dynamic(Input* in, Output* out) {
    const int P = rt_.world;
    hipStream_t st = rt_.stream;
    double* Xd = X_.get(N_ * A_ + 1);
    int* Ld = lab_.get(N_ + 1);
    double* Qd = Qx_.get(Q_ * A_ + 1);
    if (rt_.rank == 0) {
      HIPCHK(hipMemcpyAsync(Xd, in->X.data(), N_ * A_ * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(Ld, in->labels.data(), N_ * 4, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(Qd, in->Qx.data(), Q_ * A_ * 8, hipMemcpyHostToDevice, st));
      // zero the counter for this call (exclusive epoch on our own window)
      const int64_t zero = 0;
      MPI_Win_lock(MPI_LOCK_EXCLUSIVE, 0, 0, ctr_win_);
      MPI_Put(&zero, 1, MPI_INT64_T, 0, 0, 1, MPI_INT64_T, ctr_win_);
      MPI_Win_unlock(0, ctr_win_);
    }
    trace.mark("h2d");
    std::vector<int> k(Q_);
    if (rt_.rank == 0) k = in->k;
    MPI_Bcast(k.data(), (int)Q_, MPI_INT, 0, MPI_COMM_WORLD);  // also orders the reset first
    if (P > 1) {
      bcast(Xd, N_ * A_);
      bcast(Ld, N_);
      bcast(Qd, Q_ * A_);
    }
    trace.mark("distribute");
    int* lb = labout_.get(Q_ + 1);
    uint64_t* cs = cs_.get(Q_ + 1);
    HIPCHK(hipMemsetAsync(lb, 0, Q_ * sizeof(int), st));
    HIPCHK(hipMemsetAsync(cs, 0, Q_ * sizeof(uint64_t), st));
    const char* e = getenv("KNN_CHUNKS_PER_RANK");
    const int per_rank = std::max(1, e ? std::atoi(e) : 4);
    const int64_t nchunks = std::max<int64_t>(1, std::min<int64_t>(Q_, (int64_t)P * per_rank));
    const int64_t csz = (Q_ + nchunks - 1) / nchunks;
    double* dd = d_.get(std::max<int64_t>(1, csz) * kmax_);
    int* ii = ids_.get(std::max<int64_t>(1, csz) * kmax_);
    int64_t done = 0;
    for (;;) {
      const int64_t c = claim();
      if (c >= nchunks) break;
      const int64_t a = c * csz, b = std::min<int64_t>(Q_, a + csz);
      if (a >= b) continue;
      local_knn(Xd, N_, Qd + a * A_, b - a, k.data() + a, dd, ii, Ld, lb + a, cs + a);
      done += b - a;
    }
    chunks_done_ = done;
    trace.mark("compute");
    if (P > 1) {
      reduce_sum_to_root(lb, Q_, MPI_INT, ncclInt32);
      reduce_sum_to_root(cs, Q_, MPI_UINT64_T, ncclUint64);
    }
    trace.mark("reduce");
    if (rt_.rank == 0) render(out, cs, lb, dd, ii);
    trace.mark("report");
    rt_.sync();
  }

 public:
  int64_t chunks_done_ = 0;  // queries this rank computed in the last dynamic call

 private:
  // ---------------------------------------------------------------- shard_gather / shard_reduce
  void sharded(Input* in, Output* out, bool tree) {
    const int P = rt_.world;
    std::vector<int64_t> cnt, off;
    block_partition(N_, P, cnt, off);
    hipStream_t st = rt_.stream;
    const int64_t nl = cnt[rt_.rank];
    double* Xd = X_.get((rt_.rank == 0 ? N_ : nl) * A_ + 1);
    double* Qd = Qx_.get(Q_ * A_ + 1);
    int* Ld = lab_.get(N_ + 1);
    if (rt_.rank == 0) {
      HIPCHK(hipMemcpyAsync(Xd, in->X.data(), N_ * A_ * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(Qd, in->Qx.data(), Q_ * A_ * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(Ld, in->labels.data(), N_ * 4, hipMemcpyHostToDevice, st));
    }
    trace.mark("h2d");
    std::vector<int> k(Q_);
    if (rt_.rank == 0) k = in->k;
    MPI_Bcast(k.data(), (int)Q_, MPI_INT, 0, MPI_COMM_WORLD);
    if (P > 1) {
      grp_start();  // MPI_Scatterv of the shards -> direct sends
      if (rt_.rank == 0) {
        for (int r = 1; r < P; ++r)
          if (cnt[r]) snd(Xd + off[r] * A_, cnt[r] * A_, r);
      } else if (nl) {
        rcv(Xd, nl * A_, 0);
      }
      grp_end();
      bcast(Qd, Q_ * A_);
    }
    trace.mark("distribute");
    const int64_t L = (int64_t)Q_ * kmax_;
    double* dd = d_.get(L);
    int* ii = ids_.get(L);
    local_knn(Xd, nl, Qd, Q_, k.data(), dd, ii, nullptr, nullptr, nullptr);
    trace.mark("compute");
    DMLPCHK(dmlp_offset_ids(ii, L, (int)off[rt_.rank], st));
    int* kd = kd_.get(Q_);
    HIPCHK(hipMemcpyAsync(kd, k.data(), Q_ * 4, hipMemcpyHostToDevice, st));
    if (P > 1 && !tree) {  // bench_1: ONE batched gather of all lists, K-way merge at the root
      double* all_d = dall_.get(rt_.rank == 0 ? L * P : 1);
      int* all_i = iall_.get(rt_.rank == 0 ? L * P : 1);
      grp_start();
      if (rt_.rank == 0) {
        HIPCHK(hipMemcpyAsync(all_d, dd, L * 8, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(all_i, ii, L * 4, hipMemcpyDeviceToDevice, st));
        for (int r = 1; r < P; ++r) {
          rcv(all_d + r * L, L, r);
          rcv(all_i + r * L, L, r);
        }
      } else {
        snd(dd, L, 0);
        snd(ii, L, 0);
      }
      grp_end();
      if (rt_.rank == 0) DMLPCHK(dmlp_merge(all_d, all_i, P, L, kmax_, kd, (int)Q_, dd, ii, kmax_, st));
    } else if (P > 1) {  // bench_2/3: binomial tree, pairwise merge at every receiving rank
      double* sd = stage_d_.get(2 * L);
      int* si = stage_i_.get(2 * L);
      for (int step = 1; step < P; step *= 2) {
        if (rt_.rank % (2 * step) == step) {
          grp_start();
          snd(dd, L, rt_.rank - step);
          snd(ii, L, rt_.rank - step);
          grp_end();
          break;
        }
        if (rt_.rank % (2 * step) == 0 && rt_.rank + step < P) {
          HIPCHK(hipMemcpyAsync(sd, dd, L * 8, hipMemcpyDeviceToDevice, st));
          HIPCHK(hipMemcpyAsync(si, ii, L * 4, hipMemcpyDeviceToDevice, st));
          grp_start();
          rcv(sd + L, L, rt_.rank + step);
          rcv(si + L, L, rt_.rank + step);
          grp_end();
          DMLPCHK(dmlp_merge(sd, si, 2, L, kmax_, kd, (int)Q_, dd, ii, kmax_, st));
        }
      }
    }
    trace.mark("merge");
    if (rt_.rank == 0) {
      int* lb = labout_.get(Q_ + 1);
      uint64_t* cs = cs_.get(Q_ + 1);
      DMLPCHK(dmlp_finalize(dd, ii, kmax_, kd, nullptr, (int)Q_, Ld, lo_, hi_, lb, cs, st));
      render(out, cs, lb, dd, ii);
      trace.mark("report");
    }
    rt_.sync();
  }

  // ---------------------------------------------------------------- grid2d (student engine.cpp)
  // R x C process grid (MPI_Dims_create): data split over grid rows, queries over grid columns,
  // rank (r, c) = r*C + c computes query block c against data shard r.  The reference's
  // two-hop scatter+row/column broadcasts become one direct xGMI send per rank from the root
  // (xGMI is a full point-to-point mesh); the lists of column c are merged at (0, c), which
  // votes and returns (label, checksum) to rank 0.  Fixes D1 (vote on the merged lists) and
  // D3 (rank 0 prints everything, in query order).
  void grid2d(Input* in, Output* out) {
    const int P = rt_.world;
    int dims[2] = {0, 0};
    MPI_Dims_create(P, 2, dims);
    const int R = dims[0], C = dims[1];
    const int row = rt_.rank / C, col = rt_.rank % C;
    std::vector<int64_t> dc, doff, qc, qoff;
    block_partition(N_, R, dc, doff);
    block_partition(Q_, C, qc, qoff);
    hipStream_t st = rt_.stream;
    const bool root = rt_.rank == 0;
    double* Xd = X_.get((root ? N_ : dc[row]) * A_ + 1);
    double* Qd = Qx_.get((root ? Q_ : qc[col]) * A_ + 1);
    int* Ld = lab_.get(N_ + 1);
    if (root) {
      HIPCHK(hipMemcpyAsync(Xd, in->X.data(), N_ * A_ * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(Qd, in->Qx.data(), Q_ * A_ * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(Ld, in->labels.data(), N_ * 4, hipMemcpyHostToDevice, st));
    }
    trace.mark("h2d");
    std::vector<int> k(Q_);
    if (root) k = in->k;
    MPI_Bcast(k.data(), (int)Q_, MPI_INT, 0, MPI_COMM_WORLD);
    if (P > 1) {
      grp_start();
      if (root) {
        for (int r = 1; r < P; ++r) {
          const int rr = r / C, cc = r % C;
          if (dc[rr]) snd(Xd + doff[rr] * A_, dc[rr] * A_, r);
          if (qc[cc]) snd(Qd + qoff[cc] * A_, qc[cc] * A_, r);
          if (rr == 0 && N_) snd(Ld, N_, r);
        }
      } else {
        if (dc[row]) rcv(Xd, dc[row] * A_, 0);
        if (qc[col]) rcv(Qd, qc[col] * A_, 0);
        if (row == 0 && N_) rcv(Ld, N_, 0);
      }
      grp_end();
    }
    trace.mark("distribute");
    const int64_t nq = qc[col];
    const int64_t L = nq * kmax_;
    const int64_t Lmax = (root ? Q_ : nq) * kmax_ + 1;
    double* dd = d_.get(Lmax);
    int* ii = ids_.get(Lmax);
    const int* kh = k.data() + qoff[col];
    local_knn(Xd, dc[row], Qd, nq, kh, dd, ii, nullptr, nullptr, nullptr);
    trace.mark("compute");
    DMLPCHK(dmlp_offset_ids(ii, L, (int)doff[row], st));
    int* kd = kd_.get(nq + 1);
    HIPCHK(hipMemcpyAsync(kd, kh, nq * 4, hipMemcpyHostToDevice, st));
    if (R > 1 && L) {  // column merge at (0, col)
      if (row == 0) {
        double* all_d = dall_.get(L * R);
        int* all_i = iall_.get(L * R);
        HIPCHK(hipMemcpyAsync(all_d, dd, L * 8, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(all_i, ii, L * 4, hipMemcpyDeviceToDevice, st));
        grp_start();
        for (int r = 1; r < R; ++r) {
          rcv(all_d + r * L, L, r * C + col);
          rcv(all_i + r * L, L, r * C + col);
        }
        grp_end();
        DMLPCHK(dmlp_merge(all_d, all_i, R, L, kmax_, kd, (int)nq, dd, ii, kmax_, st));
      } else {
        grp_start();
        snd(dd, L, col);
        snd(ii, L, col);
        grp_end();
      }
    }
    trace.mark("merge");
    if (row == 0) {
      int* lb = labout_.get((root ? Q_ : nq) + 1);
      uint64_t* cs = cs_.get((root ? Q_ : nq) + 1);
      DMLPCHK(dmlp_finalize(dd, ii, kmax_, kd, nullptr, (int)nq, Ld, lo_, hi_, lb, cs, st));
      if (C > 1) {  // row-0 gather of (label, checksum [, lists]) in query order
        grp_start();
        if (root) {
          for (int c = 1; c < C; ++c) {
            if (!qc[c]) continue;
            rcv(lb + qoff[c], qc[c], c);
            rcv(cs + qoff[c], qc[c], c);
            if (debug_) {
              rcv(dd + qoff[c] * kmax_, qc[c] * kmax_, c);
              rcv(ii + qoff[c] * kmax_, qc[c] * kmax_, c);
            }
          }
        } else if (nq) {
          snd(lb, nq, 0);
          snd(cs, nq, 0);
          if (debug_) {
            snd(dd, L, 0);
            snd(ii, L, 0);
          }
        }
        grp_end();
      }
      trace.mark("gather");
      if (root) render(out, cs, lb, dd, ii);
      trace.mark("report");
    }
    rt_.sync();
  }

  // ---------------------------------------------------------------- ring
  // The long-context analog (parallel/strategies.py ring): the dataset is sharded N/P per GPU and
  // never replicated, the queries are split in P blocks, and every rank keeps the running top-k
  // of its block while the shards travel one hop per step around the ring.  Each exchange runs
  // on a side stream while the local screen + exact re-rank of the shard in hand runs on the
  // engine stream; the running and new lists are merged by the K-way merge kernel.  Memory per
  // GPU: two shards + Q/P queries.
  DevBuf<double> ring_a_, ring_b_, ring_d_;
  DevBuf<int> ring_i_;
  hipStream_t ring_st_ = nullptr;
  hipEvent_t ring_ev_ = nullptr, ring_done_ = nullptr;
  void ring(Input* in, Output* out) {
    const int P = rt_.world, r = rt_.rank;
    std::vector<int64_t> nc, nd, qc, qd;
    block_partition(N_, P, nc, nd);
    block_partition(Q_, P, qc, qd);
    const int64_t mx = *std::max_element(nc.begin(), nc.end());
    hipStream_t st = rt_.stream;
    if (P > 1 && !ring_st_) {
      HIPCHK(hipStreamCreateWithFlags(&ring_st_, hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&ring_ev_, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&ring_done_, hipEventDisableTiming));
    }
    double* cur = ring_a_.get(mx * A_ + 1);
    double* nxt = ring_b_.get(mx * A_ + 1);
    const int64_t nq = qc[r];
    double* Qd = Qx_.get((r == 0 ? Q_ : nq) * A_ + 1);
    int* Ld = lab_.get(N_ + 1);
    double* Xall = r == 0 ? X_.get(N_ * A_ + 1) : nullptr;
    if (r == 0) {
      HIPCHK(hipMemcpyAsync(Xall, in->X.data(), N_ * A_ * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(Qd, in->Qx.data(), Q_ * A_ * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(Ld, in->labels.data(), N_ * 4, hipMemcpyHostToDevice, st));
      if (nc[0]) HIPCHK(hipMemcpyAsync(cur, Xall, nc[0] * A_ * 8, hipMemcpyDeviceToDevice, st));
    }
    trace.mark("h2d");
    std::vector<int> kl(std::max<int64_t>(1, nq)), sc(P), so(P);
    for (int i = 0; i < P; ++i) { sc[i] = (int)qc[i]; so[i] = (int)qd[i]; }
    MPI_Scatterv(r == 0 ? in->k.data() : nullptr, sc.data(), so.data(), MPI_INT, kl.data(), sc[r],
                 MPI_INT, 0, MPI_COMM_WORLD);
    if (P > 1) {
      grp_start();  // shards and query blocks: one direct hop each from the root
      if (r == 0) {
        for (int t = 1; t < P; ++t) {
          if (nc[t]) snd(Xall + nd[t] * A_, nc[t] * A_, t);
          if (qc[t]) snd(Qd + qd[t] * A_, qc[t] * A_, t);
        }
      } else {
        if (nc[r]) rcv(cur, nc[r] * A_, 0);
        if (nq) rcv(Qd, nq * A_, 0);
      }
      grp_end();
      bcast(Ld, N_);  // the vote needs every label
    }
    trace.mark("distribute");
    const int64_t L = std::max<int64_t>(1, nq) * kmax_;
    double* sd = ring_d_.get(2 * L);  // [running | this shard's] lists, merged in place below
    int* si = ring_i_.get(2 * L);
    double* dd = d_.get(L);
    int* ii = ids_.get(L);
    int* kd = kd_.get(std::max<int64_t>(1, nq));
    if (nq) HIPCHK(hipMemcpyAsync(kd, kl.data(), nq * 4, hipMemcpyHostToDevice, st));
    bool have = false;
    for (int step = 0; step < P; ++step) {
      const int src = (r + P - step) % P;  // the shard in hand started on rank src
      if (step < P - 1) {
        // the exchange reads cur / fills nxt on the side stream, concurrently with the compute
        HIPCHK(hipEventRecord(ring_ev_, st));  // cur complete (received / staged) on st
        HIPCHK(hipStreamWaitEvent(ring_st_, ring_ev_, 0));
        ring_exchange(cur, nxt, mx * A_, ring_st_);
        HIPCHK(hipEventRecord(ring_done_, ring_st_));
      }
      if (nq && nc[src]) {
        double* od = have ? sd + L : sd;
        int* oi = have ? si + L : si;
        local_knn(cur, nc[src], Qd, nq, kl.data(), od, oi, nullptr, nullptr, nullptr);
        DMLPCHK(dmlp_offset_ids(oi, L, (int)nd[src], st));
        if (have) {
          DMLPCHK(dmlp_merge(sd, si, 2, L, kmax_, kd, (int)nq, dd, ii, kmax_, st));
          HIPCHK(hipMemcpyAsync(sd, dd, L * 8, hipMemcpyDeviceToDevice, st));
          HIPCHK(hipMemcpyAsync(si, ii, L * 4, hipMemcpyDeviceToDevice, st));
        }
        have = true;
      }
      if (step < P - 1) {
        HIPCHK(hipStreamWaitEvent(st, ring_done_, 0));  // nxt landed; cur free to overwrite
        std::swap(cur, nxt);
      }
    }
    if (nq && !have) {  // no data at all (N == 0): padding lists
      HIPCHK(hipMemsetAsync(si, 0xff, L * 4, st));
      DMLPCHK(dmlp_fill_f64(sd, L, INFINITY, st));
    }
    trace.mark("compute");
    int* lb = labout_.get((r == 0 ? Q_ : nq) + 1);
    uint64_t* cs = cs_.get((r == 0 ? Q_ : nq) + 1);
    if (nq)
      DMLPCHK(dmlp_finalize(sd, si, kmax_, kd, nullptr, (int)nq, Ld, lo_, hi_, lb, cs, st));
    if (P > 1) {  // (label, checksum [, lists]) to rank 0 in query order
      double* gd = r == 0 ? dall_.get(Q_ * kmax_ + 1) : nullptr;
      int* gi = r == 0 ? iall_.get(Q_ * kmax_ + 1) : nullptr;
      if (r == 0 && debug_ && nq) {
        HIPCHK(hipMemcpyAsync(gd, sd, nq * kmax_ * 8, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(gi, si, nq * kmax_ * 4, hipMemcpyDeviceToDevice, st));
      }
      grp_start();
      if (r == 0) {
        for (int t = 1; t < P; ++t) {
          if (!qc[t]) continue;
          rcv(lb + qd[t], qc[t], t);
          rcv(cs + qd[t], qc[t], t);
          if (debug_) {
            rcv(gd + qd[t] * kmax_, qc[t] * kmax_, t);
            rcv(gi + qd[t] * kmax_, qc[t] * kmax_, t);
          }
        }
      } else if (nq) {
        snd(lb, nq, 0);
        snd(cs, nq, 0);
        if (debug_) {
          snd(sd, nq * kmax_, 0);
          snd(si, nq * kmax_, 0);
        }
      }
      grp_end();
      trace.mark("gather");
      if (r == 0) render(out, cs, lb, gd, gi);
    } else {
      render(out, cs, lb, sd, si);
    }
    trace.mark("report");
    rt_.sync();
  }

  // ---------------------------------------------------------------- serial (bench.debug)
  void serial(Input* in, Output* out) {
    if (rt_.rank != 0) return;
    out->kstride = kmax_;
    out->dist.assign(Q_ * kmax_, INFINITY);
    out->ids.assign(Q_ * kmax_, -1);
    DMLPCHK(dmlp_kdtree_knn(in->X.data(), N_, A_, in->Qx.data(), Q_, in->k.data(), kmax_,
                            out->dist.data(), out->ids.data()));
    trace.mark("kdtree");
    out->label.resize(Q_);
    out->cs.resize(Q_);
    DMLPCHK(dmlp_cpu_finalize(out->dist.data(), out->ids.data(), kmax_, in->k.data(), Q_,
                              in->labels.data(), out->label.data(), out->cs.data()));
    trace.mark("vote");
    if (!debug_) {
      out->report.resize(48 * Q_ + 64);
      out->report.resize(dmlp_cpu_format_report(out->cs.data(), Q_, 0, out->report.data()));
    }
  }
};

template <> inline ncclDataType_t KnnCore::nty<double>() { return ncclFloat64; }
template <> inline ncclDataType_t KnnCore::nty<int>() { return ncclInt32; }
template <> inline ncclDataType_t KnnCore::nty<uint64_t>() { return ncclUint64; }

// KNN_METRICS=<path>: JSON sidecar written by rank 0 after the run (SURVEY.md §5 metrics row).
inline void write_metrics(const char* path, const std::string& strategy, const Runtime& rt, const Input& in,
                   double ms, const std::vector<std::pair<std::string, double>>& phases,
                   int64_t bytes_total) {
  FILE* f = std::fopen(path, "w");
  if (!f) return;
  int kmax = 0;
  for (int k : in.k) kmax = std::max(kmax, k);
  std::fprintf(f, "{\"engine\": \"knn_engine\", \"strategy\": \"%s\", \"ranks\": %d, \"N\": %lld, "
               "\"Q\": %lld, \"A\": %d, \"kmax\": %d, \"time_ms\": %.3f, \"queries_per_s\": %.1f, "
               "\"bytes_on_wire\": %lld, \"effective_GBps\": %.3f, \"phases_ms_rank0\": {",
               strategy.c_str(), rt.world, (long long)in.N, (long long)in.Q, in.A, kmax, ms,
               ms > 0 ? in.Q / (ms * 1e-3) : 0.0, (long long)bytes_total,
               ms > 0 ? bytes_total / (ms * 1e-3) / 1e9 : 0.0);
  for (size_t i = 0; i < phases.size(); ++i)
    std::fprintf(f, "%s\"%s\": %.3f", i ? ", " : "", phases[i].first.c_str(), phases[i].second);
  std::fprintf(f, "}}\n");
  std::fclose(f);
}


}  // namespace dmlp_rt
