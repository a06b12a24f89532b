// create_proof for the constraint system of the reference's MstInclusionCircuit, driven from C++ over the C ABI
// (include/summa_gpu.h): the compiled-host counterpart of circuits_halo2_amd/prover.py, same steps, same transcript,
// same 2144-byte proof [REF zk_prover/src/circuits/utils.rs:94-101 -> halo2_proofs::plonk::create_proof with
// ProverSHPLONK; proof layout and Keccak transcript: contracts/src/InclusionVerifier.sol:85-110, 274-367].
// Every data-parallel step runs on the device; the host does what upstream also does serially (transcript, the
// lookup's sort, scalars of the multi-open, blinding factors from the OS entropy source).
// The circuit-specific inputs -- fixed / permutation columns, the GraphEvaluator programs of the gates and of the
// lookup input -- come from the proving key (here: a bundle file written by circuits_halo2_amd.prover.export_bundle).
// This header holds what needs the HIP runtime: the per-thread session and column pool, the proving key's device forms
// and the driver (ProofRun: one member function per phase).  The host arithmetic lives in three headers that build
// without it: summa_fr.hpp (Fr, the Fq byte conversion), summa_transcript.hpp (Keccak-256, Blake2b, both transcripts)
// and summa_proof_host.hpp (the constraint system's shape, the lookup permutation, the multi-open's scalars).
// Header-only.  Proofs are checked by tests/test_gpu_prover.py, the host arithmetic by tests/test_proof_host_cpu.py.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <functional>
#include <exception>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "summa_gpu.h"
#include "summa_fr.hpp"
#include "summa_transcript.hpp"
#include "summa_proof_host.hpp"

namespace summa {
namespace prover {

static_assert(COL_FIXED == SG_VS_FIXED && COL_ADVICE == SG_VS_ADVICE && COL_INSTANCE == SG_VS_INSTANCE,
              "summa_proof_host.hpp's permutation table speaks the C ABI's column kinds");

struct Options {
  bool sanity_checks = true;   // refuse a witness whose permutation / lookup grand product does not close (upstream's cargo
                               // feature), or whose advice words are not canonical field elements
  const uint8_t* blinding_key = nullptr;   // tests only: 32 bytes, the ChaCha20 key of the blinding values; null: the OS entropy source
};
struct WitnessError : std::runtime_error {   // the assignment, not the machinery, is at fault
  using std::runtime_error::runtime_error;
};

// ------------------------------------------------------------------ inputs
struct Graph {  // a GraphEvaluator program as the C ABI takes it
  std::vector<uint8_t> constants;
  std::vector<int32_t> rotations;
  std::vector<sg_calculation> calculations;
  std::vector<sg_value_source> parts;
  sg_graph view() const {
    return sg_graph{constants.data(), (uint32_t)(constants.size() / 32), rotations.data(), (uint32_t)rotations.size(),
                    calculations.data(), (uint32_t)calculations.size(), parts.data(), (uint32_t)parts.size()};
  }
};

inline void ck(int rc, const char* what) {
  if (rc != SG_OK) throw std::runtime_error(std::string(what) + ": " + sg_last_error());
}
inline void hk(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
// Per-thread prover state: the stream proofs of this thread run on, two side streams with their fork / join events,
// the pool of freed device columns and the page-locked staging area.  Nothing is shared between host threads, so
// several proofs can be in flight on one GPU (one thread each, circuits_halo2_amd/batch.py); the C ABI underneath
// gives every concurrent call its own lane.
inline bool& session_gone() {   // trivially destructible, so still readable after this thread's Session has been destroyed
  static thread_local bool gone = false;
  return gone;
}
// What a host thread's session leaves behind when the thread ends.  A thread-local destructor must not call into HIP: worker
// threads are joined while the process shuts down, and hipFree from a thread's destructor then runs into the runtime's own
// teardown (seen as a crash in amd::Context::svmFree with more worker threads than lanes).  So a dying session hands its
// device columns, streams, events and pinned staging to this process-wide store; the next session on another thread takes
// them from here before asking the runtime, and release_orphans() (sg_shutdown, with the device idle) returns them.
struct Orphans {
  std::mutex mu;
  std::multimap<size_t, void*> pool;
  std::vector<hipStream_t> streams;
  std::vector<hipEvent_t> events;
  std::vector<std::pair<uint64_t*, size_t>> pinned;
};
inline Orphans& orphans() {
  static Orphans* o = new Orphans();   // never destroyed: sessions may end after static destruction has begun
  return *o;
}
inline void release_orphans() {
  Orphans& o = orphans();
  std::lock_guard<std::mutex> lk(o.mu);
  for (auto& kv : o.pool) (void)hipFree(kv.second);
  for (auto& p : o.pinned) (void)hipHostFree(p.first);
  for (auto& st : o.streams) (void)hipStreamDestroy(st);
  for (auto& e : o.events) (void)hipEventDestroy(e);
  o.pool.clear();
  o.pinned.clear();
  o.streams.clear();
  o.events.clear();
}
struct Session {
  hipStream_t main = nullptr;                 // NULL: HIP's default stream (single-threaded callers)
  hipStream_t side[2] = {nullptr, nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
  std::multimap<size_t, void*> pool;          // freed columns are kept for the next proof (hipMalloc / hipFree synchronise the device)
  uint64_t* pinned = nullptr;
  size_t pinned_cap = 0;
  uint64_t* pinned_small = nullptr;           // 8 rows of page-locked memory, mapped into the device: small values the kernels write
                                              // there themselves (checked where the host waits anyway; no copy launches)
  uint8_t* pinned_small_dev = nullptr;        // ... its device address
  ~Session() {   // no HIP calls here (see Orphans)
    Orphans& o = orphans();
    std::lock_guard<std::mutex> lk(o.mu);
    for (auto& kv : pool) o.pool.emplace(kv.first, kv.second);
    if (pinned) o.pinned.emplace_back(pinned, pinned_cap);
    if (pinned_small) o.pinned.emplace_back(pinned_small, (size_t)0);   // (capacity 0: released, never handed on as row staging)
    for (auto& st : side)
      if (st) o.streams.push_back(st);
    if (ev_fork) o.events.push_back(ev_fork);
    for (auto& e : ev_join)
      if (e) o.events.push_back(e);
    session_gone() = true;
  }
};
inline Session& session() {
  static thread_local Session s;
  return s;
}
// a stream / an event for a new session: one an ended session left behind, else a new one
inline hipStream_t adopt_or_create_stream(int priority) {
  {
    Orphans& o = orphans();
    std::lock_guard<std::mutex> lk(o.mu);
    if (!o.streams.empty()) {
      hipStream_t st = o.streams.back();
      o.streams.pop_back();
      return st;
    }
  }
  hipStream_t st = nullptr;
  hk(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, priority), "stream");
  return st;
}
inline hipEvent_t adopt_or_create_event() {
  {
    Orphans& o = orphans();
    std::lock_guard<std::mutex> lk(o.mu);
    if (!o.events.empty()) {
      hipEvent_t e = o.events.back();
      o.events.pop_back();
      return e;
    }
  }
  hipEvent_t e = nullptr;
  hk(hipEventCreateWithFlags(&e, hipEventDisableTiming), "event");
  return e;
}
inline hipStream_t main_stream() { return session().main; }
struct StreamScope {   // run this thread's prover calls on `s` for the scope
  hipStream_t prev;
  explicit StreamScope(hipStream_t s) : prev(session().main) { session().main = s; }
  ~StreamScope() { session().main = prev; }
};
inline std::multimap<size_t, void*>& column_pool() { return session().pool; }
inline void release_column_pool() {
  for (auto& kv : column_pool()) (void)hipFree(kv.second);
  column_pool().clear();
}
inline void d2h(void* host, const void* dev, size_t bytes) {   // ordered on the thread's main stream, complete on return
  // (the stream is drained by the library's wait FIRST -- asleep when "host.wait_sleep_us" is set: a copy into pageable memory
  // waits for everything ahead of it inside hipMemcpyAsync, busily; csrc/host_wait.h, host_copy_d2h)
  ck(sg_stream_wait(main_stream()), "sync");
  hk(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, main_stream()), "D2H");
  ck(sg_stream_wait(main_stream()), "sync");
}
inline void h2d(void* dev, const void* host, size_t bytes) {
  hk(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, main_stream()), "H2D");
  ck(sg_stream_wait(main_stream()), "sync");   // the host buffer may be a temporary
}
struct DevCol {  // device column of Fr (Montgomery); owned unless borrowed from the caller
  void* p = nullptr;
  size_t rows = 0;
  bool owned = true;
  DevCol() = default;
  static DevCol borrow(void* ptr, size_t r) {
    DevCol c;
    c.p = ptr;
    c.rows = r;
    c.owned = false;
    return c;
  }
  explicit DevCol(size_t r) : rows(r) {
    auto it = column_pool().find(r);
    if (it != column_pool().end()) {
      p = it->second;
      column_pool().erase(it);
    } else {
      {
        Orphans& o = orphans();
        std::lock_guard<std::mutex> lk(o.mu);
        auto ot = o.pool.find(r);
        if (ot != o.pool.end()) {
          p = ot->second;
          o.pool.erase(ot);
        }
      }
      if (!p) hk(hipMalloc(&p, 32 * r), "hipMalloc");
    }
  }
  DevCol(const DevCol&) = delete;
  DevCol& operator=(const DevCol&) = delete;
  DevCol(DevCol&& o) noexcept : p(o.p), rows(o.rows), owned(o.owned) { o.p = nullptr; }
  void give_back() {   // to this thread's pool; objects that outlive the thread's session (process exit) just let go
    if (p && owned && !session_gone()) column_pool().emplace(rows, p);
    p = nullptr;
  }
  DevCol& operator=(DevCol&& o) noexcept {
    give_back();
    p = o.p;
    rows = o.rows;
    owned = o.owned;
    o.p = nullptr;
    return *this;
  }
  ~DevCol() { give_back(); }
  uint8_t* at(size_t row) const { return static_cast<uint8_t*>(p) + 32 * row; }
  void upload(const void* host, size_t first, size_t count) { h2d(at(first), host, 32 * count); }
  void zero() { hk(hipMemsetAsync(p, 0, 32 * rows, main_stream()), "memset"); }
};

inline std::vector<void*> ptrs(const std::vector<DevCol>& cols) {
  std::vector<void*> p;
  for (auto& c : cols) p.push_back(c.p);
  return p;
}
// coefficient form (iNTT; the Lagrange columns stay) and coset-major extended form of a group of columns: new columns,
// appended to `coeff` / `ext`.  Batched launches hold at most 16 vectors
inline void to_coeff_and_cosets(const std::vector<void*>& lag, uint32_t k, uint32_t ext_k, const uint8_t omega_inv[32], const uint8_t n_inv[32],
                                std::vector<DevCol>& coeff, std::vector<DevCol>& ext, hipStream_t st) {
  const size_t n = (size_t)1 << k;
  std::vector<void*> pc, pe;
  for (size_t i = 0; i < lag.size(); i++) {
    coeff.emplace_back(n);
    ext.emplace_back(n * QUOTIENT_PIECES);
    pc.push_back(coeff.back().p);
    pe.push_back(ext.back().p);
  }
  for (size_t i = 0; i < pc.size(); i += 16) {
    const size_t m = std::min<size_t>(16, pc.size() - i);
    ck(sg_ntt_fr_batch_oop_dev(lag.data() + i, pc.data() + i, m, omega_inv, n_inv, k, st), "iNTT batch");
    ck(sg_coeff_to_cosets_batch_dev(pc.data() + i, pe.data() + i, m, k, ext_k, QUOTIENT_PIECES, st), "coset NTT batch");
  }
}

struct ProvingKey {
  std::vector<uint64_t> table_rows;  // the lookup table column (fixed 4), canonical limbs of the usable rows (host copy)
  bool table_is_range = false;       // ... every usable row below 2^16: the device-side permutation applies (known with the key)
  uint32_t k = 0;
  size_t n = 0, usable = 0;
  uint64_t srs = 0;
  uint8_t vk_digest_be[32] = {0};
  Graph gates, lookup_input;
  // the challenges the gate program reads: challenge i = sum over e in gate_challenge_exps[i] of y^e
  std::vector<std::vector<uint32_t>> gate_challenge_exps;
  std::vector<DevCol> fixed_lag, sigma_lag, fixed_coeff, sigma_coeff, fixed_ext, sigma_ext;
  DevCol l0_ext, l_last_ext, l_active_ext;
  uint32_t ext_k() const { return k + 3; }  // degree 6: extended domain 2^(k + 3)
  // the quotient has degree < QUOTIENT_PIECES * n: it is evaluated on that many cosets of the 2^k domain (the first ones of
  // the extended domain, coset-major: sg_coeff_to_cosets_batch_dev), not on all 2^(k + 3) points; "ext" columns have this size
  size_t ext_rows() const { return n * QUOTIENT_PIECES; }

  // fixed / sigma: Lagrange-basis device columns (moved in); builds the coefficient and extended-coset forms
  void build(uint32_t k_, uint64_t srs_, std::vector<DevCol>&& fixed, std::vector<DevCol>&& sigma) {
    k = k_;
    n = (size_t)1 << k;
    usable = n - (BLINDING + 1);
    srs = srs_;
    fixed_lag = std::move(fixed);
    sigma_lag = std::move(sigma);
    uint8_t omega_inv[32], n_inv[32];
    ck(sg_domain_constant(k, 1, omega_inv), "domain constant");
    ck(sg_domain_constant(k, 2, n_inv), "domain constant");
    std::vector<DevCol> sel;
    const Fr one = Fr::one();
    for (int s = 0; s < 3; s++) {
      sel.emplace_back(n);
      sel.back().zero();
    }
    sel[0].upload(one.l, 0, 1);
    sel[1].upload(one.l, usable, 1);
    {
      std::vector<Fr> ones(usable, one);
      sel[2].upload(ones.data(), 0, usable);
    }
    auto transform = [&](std::vector<DevCol>& lag, std::vector<DevCol>& coeff, std::vector<DevCol>& ext) {
      to_coeff_and_cosets(ptrs(lag), k, ext_k(), omega_inv, n_inv, coeff, ext, main_stream());
    };
    transform(fixed_lag, fixed_coeff, fixed_ext);
    transform(sigma_lag, sigma_coeff, sigma_ext);
    std::vector<DevCol> sel_coeff, sel_ext;
    transform(sel, sel_coeff, sel_ext);
    l0_ext = std::move(sel_ext[0]);
    l_last_ext = std::move(sel_ext[1]);
    l_active_ext = std::move(sel_ext[2]);
    {
      DevCol canon(n);
      table_rows.resize(4 * n);
      ck(sg_fr_from_montgomery_dev(fixed_lag[4].p, canon.p, n, main_stream()), "from_montgomery");
      d2h(table_rows.data(), canon.p, 32 * n);
    }
    ck(sg_stream_wait(main_stream()), "sync");
    table_is_range = true;
    for (size_t i = 0; i < usable; i++)
      table_is_range = table_is_range && table_rows[4 * i] < (1u << 16) && !(table_rows[4 * i + 1] | table_rows[4 * i + 2] | table_rows[4 * i + 3]);
  }
};

inline void os_random(uint8_t* out, size_t bytes) {
  FILE* f = std::fopen("/dev/urandom", "rb");
  if (!f || std::fread(out, 1, bytes, f) != bytes) {
    if (f) std::fclose(f);
    throw std::runtime_error("/dev/urandom");
  }
  std::fclose(f);
}

inline uint64_t* pinned_small_rows() {   // 8 rows, allocated once per session
  uint64_t*& p = session().pinned_small;
  if (!p) {
    hk(hipHostMalloc(reinterpret_cast<void**>(&p), 32 * 8, hipHostMallocMapped | hipHostMallocCoherent), "hipHostMalloc");
    hk(hipHostGetDevicePointer(reinterpret_cast<void**>(&session().pinned_small_dev), p, 0), "hipHostGetDevicePointer");
  }
  return p;
}
// rows of that block: 0 .. 2 the grand products' closing values, 3 the remainder of the final division, 4 two status words
// (range check of the advice columns, lookup permutation)
enum { MAIL_CLOSING = 0, MAIL_REMAINDER = 3, MAIL_STATUS = 4 };
inline uint8_t* pinned_small_dev_row(uint32_t row) {
  pinned_small_rows();
  return session().pinned_small_dev + 32 * row;
}
inline uint64_t* pinned_rows(size_t rows) {  // page-locked host staging, grown on demand, kept (per thread)
  uint64_t*& p = session().pinned;
  size_t& cap = session().pinned_cap;
  if (rows > cap) {
    if (p) (void)hipHostFree(p);
    hk(hipHostMalloc(reinterpret_cast<void**>(&p), 32 * rows), "hipHostMalloc");
    cap = rows;
  }
  return p;
}

struct DomainConstants {   // of the 2^k domain, from the library: omega and 1 / omega as field elements; 1 / omega and 1 / n as the ABI takes them
  uint8_t omega_inv_b[32], n_inv_b[32];
  Fr omega, omega_inv;
  explicit DomainConstants(uint32_t k) {
    ck(sg_domain_constant(k, 0, reinterpret_cast<uint8_t*>(omega.l)), "domain constant");
    ck(sg_domain_constant(k, 1, omega_inv_b), "domain constant");
    ck(sg_domain_constant(k, 2, n_inv_b), "domain constant");
    std::memcpy(omega_inv.l, omega_inv_b, 32);
  }
};

struct Timings { std::map<std::string, double> ms; };

// The main stream of the proof and two side streams: independent latency chains (the transforms of a phase under its
// commitments, the draw of the random polynomial) run next to the main stream; the library keeps its work space per stream.
// fork: the side streams wait for everything enqueued on the main stream; join: the reverse
struct Streams {
  hipStream_t ms, side[2];
  hipEvent_t ev_fork, ev_join[2];
  // Everything on the main stream: (a) a proof that is one of several in flight (between sg_commit_combine_begin / _end: the
  // batch driver) -- the other proofs are its concurrency, and every fork / join is three event records and four stream waits,
  // each a marker the runtime's completion thread has to retire (one thread per process: 3.6 ms of CPU per proof at 25 records
  // and 22 waits; without the side streams a batch of 1024 runs 2-7 % faster on a whole host and on a 1/8 share of it,
  // profiles/r04_sweeps/batch_host_cpu_profile.txt); (b) SG_PROVER_SERIAL (development aid: a kernel trace shows every kernel alone)
  bool serial;
  void fork() const {
    if (serial) return;                  // one stream: nothing to order (and no markers for the runtime to retire)
    hk(hipEventRecord(ev_fork, ms), "event");
    for (auto& st : side) hk(hipStreamWaitEvent(st, ev_fork, 0), "wait");
  }
  void join(int i) const {               // the main stream waits for side stream i
    if (serial) return;
    hk(hipEventRecord(ev_join[i], side[i]), "event");
    hk(hipStreamWaitEvent(ms, ev_join[i], 0), "wait");
  }
  void join() const {
    for (int i = 0; i < 2; i++) join(i);
  }
};
inline Streams open_streams() {   // this thread's session streams, made on its first proof
  Session& s = session();
  if (!s.side[0]) {
    {
      // the side streams carry work that is needed a phase later (transforms under a commitment job): lowest priority, so
      // that the commitment job's latency-bound kernels on the other streams are dispatched first (SG_SIDE_PRIORITY=0: normal)
      int least = 0, greatest = 0;
      (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
      const char* v = std::getenv("SG_SIDE_PRIORITY");
      const int prio = (v && v[0] == '0') ? 0 : least;
      for (auto& st : s.side) st = adopt_or_create_stream(prio);
    }
    s.ev_fork = adopt_or_create_event();
    for (auto& e : s.ev_join) e = adopt_or_create_event();
  }
  const hipStream_t ms = main_stream();
  const bool serial = std::getenv("SG_PROVER_SERIAL") != nullptr || sg_commit_combining() == 1;
  return Streams{ms, {serial ? ms : s.side[0], serial ? ms : s.side[1]}, s.ev_fork, {s.ev_join[0], s.ev_join[1]}, serial};
}
// A proof that ends in an exception (WitnessError, a failed call) may leave kernels behind on the side streams, and its
// device columns go back to this thread's pool as the stack unwinds -- the next proof would take them while those
// kernels still write to them.  On the way out by exception the three streams are drained first.
struct DrainOnUnwind {
  hipStream_t s[3];
  int depth = std::uncaught_exceptions();
  ~DrainOnUnwind() {
    if (std::uncaught_exceptions() > depth)
      for (hipStream_t st : s) (void)hipStreamSynchronize(st);
  }
};
// SG_PROVER_TRACE=1: the host's own timeline (no synchronisation added): when each step of the driver was reached
struct HostTrace {
  const bool on = std::getenv("SG_PROVER_TRACE") != nullptr;
  const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
  std::vector<std::pair<const char*, double>> marks;
  void mark(const char* what) {
    if (on) marks.emplace_back(what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_begin).count());
  }
  ~HostTrace() {
    double prev = 0;
    for (auto& kv : marks) {
      std::fprintf(stderr, "  %9.1f us (+%7.1f)  %s\n", kv.second, kv.second - prev, kv.first);
      prev = kv.second;
    }
  }
};

// One proof: what lives across the phases of create_proof, and the phases.  prove() is the transcript's order; each phase
// enqueues its work, commits, and writes its points or scalars.  Every device column is a member: all of them live until
// the proof is done (returning one to the pool earlier would hand a buffer on while kernels may still write to it, or
// need a host sync).
template <class Transcript>
struct ProofRun {
  const ProvingKey& pk;
  std::vector<DevCol>& advice;   // 3 device columns (Lagrange, n rows; the last 6 rows are overwritten with blinding values)
  const std::vector<Fr>& instances;
  Transcript& tr;
  const Options& opt;
  Timings* const timings;
  const uint32_t k = pk.k, ext_k = pk.ext_k();
  const size_t n = pk.n, u = pk.usable, ne = pk.ext_rows();
  std::chrono::steady_clock::time_point clock = std::chrono::steady_clock::now();
  HostTrace trace;
  const DomainConstants dom{k};
  // blinding values: a 32-byte key from the OS per proof, expanded by ChaCha20 on the device; one stream id per draw
  const std::array<uint8_t, 32> key = blinding_key(opt);
  uint64_t draws = 0;
  const Streams st = open_streams();
  DrainOnUnwind drain_on_unwind{{st.side[0], st.side[1], st.ms}};
  const sg_graph g_in = pk.lookup_input.view(), g_gates = pk.gates.view();
  const std::vector<RotationSet> sets = rotation_sets();

  // columns (members: see above) and what later phases read of the earlier ones
  DevCol pin, ptab, instance_col, random_poly, inp, lz, values, f_all, l_poly, w2;
  std::vector<DevCol> co1, ex1, zs, co3, ex3, pieces_col, fs, quotients;
  std::vector<uint8_t> pts1;             // phase 1's commitments: a0 a1 a2 a' s' random
  std::vector<void*> pieces;
  std::map<Key, void*> poly;             // coefficient forms, for the evaluations and the multi-open
  Fr theta, beta, gamma, y, x, x_n, zeta, nu;
  RotationPoints point;
  Evaluations evals;

  ProofRun(const ProvingKey& pk_, std::vector<DevCol>& advice_, const std::vector<Fr>& instances_, Transcript& tr_, const Options& opt_,
           Timings* timings_)
      : pk(pk_), advice(advice_), instances(instances_), tr(tr_), opt(opt_), timings(timings_) {}

  void lap(const char* name) {  // per-phase wall clock with the device drained, only when asked for
    if (!timings) return;
    hk(hipDeviceSynchronize(), "sync");   // timing mode only
    const auto now = std::chrono::steady_clock::now();
    timings->ms[name] += std::chrono::duration<double, std::milli>(now - clock).count();
    clock = now;
  }
  void mark(const char* what) { trace.mark(what); }
  static std::array<uint8_t, 32> blinding_key(const Options& o) {
    std::array<uint8_t, 32> key;
    if (o.blinding_key) std::memcpy(key.data(), o.blinding_key, 32);
    else os_random(key.data(), 32);
    return key;
  }
  struct Rows { DevCol* col; size_t first, count; };
  void rand_rows(std::initializer_list<Rows> list) {   // one launch; draw ids as if drawn one after the other
    void* outs[8];
    size_t counts[8];
    uint32_t m = 0;
    for (const Rows& r : list) {
      outs[m] = r.col->at(r.first);
      counts[m++] = r.count;
    }
    ck(sg_fr_random_batch_dev(key.data(), draws + 1, outs, counts, m, st.ms), "fr_random");
    draws += m;
  }
  // a draw out of turn: the values of draw number `id` (1-based, in the order upstream's prover draws) on stream `s`, for a
  // column that depends on nothing and can be filled while the device is busy with something else.  The draw numbers of
  // the others do not move, so the proof under a fixed key is the one the in-order schedule gives.
  void rand_at(uint64_t id, DevCol& col, size_t first, size_t count, hipStream_t s) {
    void* outs[1] = {col.at(first)};
    size_t counts[1] = {count};
    ck(sg_fr_random_batch_dev(key.data(), id, outs, counts, 1, s), "fr_random");
  }
  void to_coeff_ext(const std::vector<void*>& lag, std::vector<DevCol>& coeff, std::vector<DevCol>& ext, hipStream_t s) {
    to_coeff_and_cosets(lag, k, ext_k, dom.omega_inv_b, dom.n_inv_b, coeff, ext, s);
  }
  // one fused commitment job on the main stream (returns when the points are back); the caller writes them where upstream does
  std::vector<uint8_t> commit(std::vector<void*> cols, std::vector<int> basis) {
    std::vector<uint8_t> out(64 * cols.size());
    ck(sg_commit_batch_mixed_dev(pk.srs, basis.data(), cols.data(), cols.size(), n, st.ms, out.data()), "commit");
    return out;
  }
  void write_points(const std::vector<uint8_t>& pts, size_t first, size_t end) {
    for (size_t i = first; i < end; i++) tr.write_point(pts.data() + 64 * i);
  }
  void* lag_col(uint32_t kind, uint32_t idx) const {
    return kind == SG_VS_ADVICE ? advice[idx].p : kind == SG_VS_FIXED ? pk.fixed_lag[idx].p : instance_col.p;
  }

  std::vector<uint8_t> prove() {
    tr.common_scalar(Fr::from_be_bytes_reduced(pk.vk_digest_be));   // vk.hash_into(transcript)
    for (auto& v : instances) tr.common_scalar(v);
    advice_and_lookup_columns();         // one commitment job: a0 a1 a2, the lookup's a' s', the random polynomial
    write_points(pts1, 0, 3);
    theta = tr.squeeze();
    lap("1_advice");
    write_points(pts1, 3, 5);
    beta = tr.squeeze();
    gamma = tr.squeeze_again();
    lap("2_lookup");
    grand_products();                    // writes z0 z1 lz and the random polynomial's point
    y = tr.squeeze();
    st.join();
    lap("3_grand_products");
    quotient();                          // writes the five pieces
    x = tr.squeeze();
    x_n = x.pow((uint64_t)n);
    lap("4_quotient");
    evaluations();                       // writes the evaluations at x
    lap("5_evaluations");
    zeta = tr.squeeze();
    nu = tr.squeeze_again();
    mark("6: zeta, nu squeezed");
    multiopen();                         // writes W, squeezes mu, writes W'
    lap("6_multiopen");
    return tr.proof;
  }

  // -- 1: advice; 2 (computed ahead of its place in the transcript): the lookup's permuted columns
  void advice_and_lookup_columns() {
    const Fr zero = Fr::zero();
    // status words in mapped page-locked memory, written by the kernels themselves and looked at after the commitments (where the
    // host waits anyway): the range check of the advice columns, the verdict of the lookup permutation
    volatile uint32_t* status = reinterpret_cast<volatile uint32_t*>(pinned_small_rows() + 4 * MAIL_STATUS);
    uint8_t* status_dev = pinned_small_dev_row(MAIL_STATUS);
    status[0] = status[1] = 0;
    if (opt.sanity_checks) {
      const void* cols[3] = {advice[0].p, advice[1].p, advice[2].p};
      ck(sg_fr_flag_noncanonical_dev(cols, 3, n, status_dev, st.ms), "range check of the advice columns");
    }
    // blinding rows of the three advice columns AND of the two permuted lookup columns (draws 1 .. 5, in upstream's order) in one
    // launch: the permutation kernels below write rows below `u` only
    pin = DevCol(n);
    ptab = DevCol(n);
    rand_rows({{&advice[0], u, n - u}, {&advice[1], u, n - u}, {&advice[2], u, n - u}, {&pin, u, n - u}, {&ptab, u, n - u}});
    instance_col = DevCol(n);
    if (instances.size() <= 8) {   // the column = its few values then zeros: one launch, the values travel as kernel arguments
      ck(sg_fr_lincomb_low_dev(nullptr, nullptr, 0, n, instances.empty() ? nullptr : instances[0].bytes(), (uint32_t)instances.size(),
                               instance_col.p, st.ms), "instance column");
    } else {
      instance_col.zero();
      instance_col.upload(instances.data(), 0, instances.size());
    }
    st.fork();
    // under the commitments; issued FIRST: started later (after the lookup's kernels) these transforms ran into the commitment
    // job's latency-bound kernels and cost it more (0.70 -> 0.82 ms) than the earlier start of the lookup kernels gained (50 us)
    to_coeff_ext({advice[0].p, advice[1].p, advice[2].p, instance_col.p}, co1, ex1, st.side[0]);
    // the random polynomial of phase 3 (draw 9: after the three advice columns, the two permuted columns and the three grand
    // products) depends on nothing: 2^k values drawn here, under phase 1's commitment job, instead of on phase 3's critical path
    random_poly = DevCol(n);
    rand_at(9, random_poly, 0, n, st.side[1]);
    // ... and is committed with phase 1's columns (below) instead of phase 3's: the one dense column among the commitments of phases
    // 1-3 leaves the job that sits on the critical path behind the grand products (phase 3: 1.34 -> 1.0 ms) and joins one that
    // is a latency chain of witness-like columns anyway (phase 1: 1.0 -> 1.24 ms); its point enters the transcript where upstream
    // writes it.  A proof is GPU-bound by now (5.4 ms of kernel time in 5.6 ms of wall clock), so the gain is the fused job's
    // saved front end and reduction, not the overlap: committing the column from a helper thread, concurrently with phase 1's
    // job, was measured and is slower; so was upstream's order, drawing and committing it in phase 3
    // (profiles/r04_sweeps/random_polynomial_early.txt).
    // The lookup's permuted columns: this circuit's lookup has ONE input and ONE table expression, so the theta-compression is
    // the expression itself and nothing here waits for theta: the two permuted columns are committed in the SAME fused job as
    // the advice columns (one MSM group's latency instead of two) and their points enter the transcript where upstream
    // writes them, after theta has been squeezed.
    std::vector<void*> fixed_lag_p = ptrs(pk.fixed_lag), adv_lag_p = {advice[0].p, advice[1].p, advice[2].p}, inst_lag_p = {instance_col.p};
    inp = DevCol(n);   // (not cleared: the input program writes every row and reads no previous value)
    ck(sg_quotient_gates_dev(inp.p, &g_in, fixed_lag_p.data(), NUM_FIXED, adv_lag_p.data(), NUM_ADVICE, inst_lag_p.data(), 1, nullptr, 0,
                             zero.bytes(), zero.bytes(), zero.bytes(), zero.bytes(), k, k, st.ms), "lookup input");
    // range tables (a property of the key): on the device, nothing waited for -- the verdict lands in status[1]
    const int prc = pk.table_is_range ? sg_lookup_permute_small_async_dev(inp.p, pk.fixed_lag[4].p, u, pin.p, ptab.p, status_dev + 4, st.ms)
                                      : SG_ERR_UNSUPPORTED;
    if (prc == SG_ERR_UNSUPPORTED) {   // general tables: sort on the host, as upstream does
      DevCol canon(n);
      uint64_t* stage = pinned_rows(3 * n);   // page-locked staging: the three 32 n-byte transfers run at link speed
      uint64_t *h_inp = stage, *h_a = stage + 4 * n, *h_s = stage + 8 * n;
      ck(sg_fr_from_montgomery_dev(inp.p, canon.p, n, st.ms), "from_montgomery");
      d2h(h_inp, canon.p, 32 * n);
      permute_expression_pair(h_inp, pk.table_rows.data(), u, h_a, h_s);
      pin.upload(h_a, 0, u);
      ptab.upload(h_s, 0, u);
      ck(sg_fr_to_montgomery_dev(pin.p, pin.p, u, st.ms), "to_montgomery");
      ck(sg_fr_to_montgomery_dev(ptab.p, ptab.p, u, st.ms), "to_montgomery");
    } else if (prc == SG_ERR_WITNESS) {
      throw WitnessError("lookup input value not in the table");
    } else {
      ck(prc, "lookup permutation");
    }
    mark("1: lookup columns ready, commit [a0 a1 a2 a' s'] issued");
    // advice and permuted-lookup columns of this circuit are witness-like: a few thousand used rows of small values (the sparse
    // hint); the sorted columns have long constant runs -> difference form (sg_commit, basis 2); the random polynomial rides along
    const int SP = SG_BASIS_SPARSE;
    st.join(1);                            // the draw of the random polynomial (side stream 1)
    pts1 = commit({advice[0].p, advice[1].p, advice[2].p, pin.p, ptab.p, random_poly.p}, {1 | SP, 1 | SP, 1 | SP, 2 | SP, 2 | SP, 0});
    // (the commitment job has waited for the stream: the status words are final)
    if (status[1] == 1) throw WitnessError("lookup input value not in the table");
    if (status[1]) throw std::runtime_error("lookup permutation: the key's table is not a range table after all");
    if (opt.sanity_checks && status[0]) throw WitnessError("advice words >= r (not canonical Montgomery field elements)");
    mark("1: commitments back");
  }

  // -- 3: grand products (the random polynomial was drawn and committed in phase 1)
  void grand_products() {
    const int SP = SG_BASIS_SPARSE;
    // the three grand products are independent up to one scalar (z1 continues from z0's last usable value)
    zs.emplace_back(n);
    zs.emplace_back(n);
    lz = DevCol(n);
    {
      // one batched call (sg_grand_products_dev): the three products share their launches -- one inversion pass instead of
      // three latency chains --, z1 continues from z0's last usable value on the device, and nothing here waits for the device
      std::vector<void*> all_vals, all_sig;   // chunk by chunk
      uint32_t chunk_cols[2] = {0, 0};
      for (uint32_t c = 0; c < NUM_SIGMA; c++) {
        chunk_cols[c / CHUNK]++;
        all_vals.push_back(lag_col(perm_kind[c], perm_idx[c]));
        all_sig.push_back(pk.sigma_lag[c].p);
      }
      void* lookup_cols[4] = {inp.p, pk.fixed_lag[4].p, pin.p, ptab.p};
      void* z_out[3] = {zs[0].p, zs[1].p, lz.p};
      // z0[u], z1[u], lz[u] land in mapped host memory, written by the kernels that produce the row: looked at when the commitments are back
      // (cleared first: a value left by an earlier proof of this thread must never pass for this proof's)
      std::memset(pinned_small_rows() + 4 * MAIL_CLOSING, 0, 3 * 32);
      ck(sg_grand_products_closing_dev(all_vals.data(), all_sig.data(), chunk_cols, 2, lookup_cols, 1, beta.bytes(), gamma.bytes(), k, u, z_out,
                                       opt.sanity_checks ? pinned_small_dev_row(MAIL_CLOSING) : nullptr, st.ms), "grand products");
      mark("3: grand products enqueued");
    }
    uint64_t* closing = pinned_small_rows() + 4 * MAIL_CLOSING;
    rand_rows({{&zs[0], u + 1, n - u - 1}, {&zs[1], u + 1, n - u - 1}, {&lz, u + 1, n - u - 1}});
    draws += 1;                                // draw 9, the random polynomial, was made in phase 1
    st.join();                                 // (the random polynomial's stream)
    st.fork();
    to_coeff_ext({pin.p, ptab.p, zs[0].p, zs[1].p, lz.p}, co3, ex3, st.side[0]);   // under the commitments
    // the grand products stay constant wherever the ratio is 1 -- all the unused rows: three piecewise-constant columns in
    // difference form, a sparse job
    mark("3: commit [z0 z1 lz random] issued");
    write_points(commit({zs[0].p, zs[1].p, lz.p}, {2 | SP, 2 | SP, 2 | SP}), 0, 3);
    write_points(pts1, 5, 6);                  // the random polynomial's commitment, made in phase 1's job
    mark("3: commitments back");
    if (opt.sanity_checks) {   // the kernels that wrote them precede the commitment job on the main stream: complete by now
      Fr last;
      std::memcpy(last.l, closing + 4, 32);         // z1[u]: the permutation's last chunk
      if (last != Fr::one()) throw WitnessError("permutation argument not satisfied by the assignment");
      std::memcpy(last.l, closing + 8, 32);         // lz[u]
      if (last != Fr::one()) throw WitnessError("lookup argument not satisfied by the assignment");
    }
  }

  // -- 4: quotient
  // the kernels take the coset-major arrays whole (QUOTIENT_PIECES blocks of 2^k rows; a rotation is an index shift of 1 inside
  // a block): one launch each
  void quotient() {
    values = DevCol(ne);
    const std::vector<Fr> y_powers = gate_challenges(pk.gate_challenge_exps, y);
    mark("4: challenges of the gate program ready");
    for (uint32_t i = 0; i < QUOTIENT_PIECES; i++) pieces_col.emplace_back(n);
    mark("4: buffers ready");
    {
      // evaluate_h in one call: gates, permutation argument, lookup argument (its input expression on the way) -- one pass over
      // the coset rows for this circuit's programs (sg_quotient_numerator_cosets_dev); `values` needs no clearing
      std::vector<void*> fixed_e = ptrs(pk.fixed_ext), adv_e = {ex1[0].p, ex1[1].p, ex1[2].p}, inst_e = {ex1[3].p};
      std::vector<void*> col_e, sig_e, z_e = {ex3[2].p, ex3[3].p};
      for (uint32_t c = 0; c < NUM_SIGMA; c++) {
        col_e.push_back(perm_kind[c] == SG_VS_ADVICE ? ex1[perm_idx[c]].p : perm_kind[c] == SG_VS_FIXED ? pk.fixed_ext[perm_idx[c]].p : ex1[3].p);
        sig_e.push_back(pk.sigma_ext[c].p);
      }
      ck(sg_quotient_numerator_cosets_dev(values.p, &g_gates, &g_in, fixed_e.data(), NUM_FIXED, adv_e.data(), NUM_ADVICE, inst_e.data(), 1,
                                          y_powers[0].bytes(), (uint32_t)pk.gate_challenge_exps.size(), z_e.data(), 2, col_e.data(), sig_e.data(),
                                          NUM_SIGMA, CHUNK, pk.l0_ext.p, pk.l_last_ext.p, pk.l_active_ext.p, ex3[4].p, ex3[0].p, ex3[1].p,
                                          pk.fixed_ext[4].p, nullptr, beta.bytes(), gamma.bytes(), theta.bytes(), y.bytes(), k, ext_k, QUOTIENT_PIECES,
                                          BLINDING + 1, st.ms), "quotient numerator");
    }
    mark("4: numerator enqueued");
    pieces = ptrs(pieces_col);
    ck(sg_cosets_to_pieces_dev(values.p, pieces.data(), k, ext_k, QUOTIENT_PIECES, st.ms), "cosets_to_pieces");
    mark("4: pieces enqueued, commit issued");
    write_points(commit(pieces, std::vector<int>(QUOTIENT_PIECES, 0)), 0, QUOTIENT_PIECES);
    mark("4: commitments back");
  }

  // -- 5: evaluations
  void evaluations() {
    for (uint32_t j = 0; j < NUM_ADVICE; j++) poly[{A_, j}] = co1[j].p;
    for (uint32_t j = 0; j < NUM_FIXED; j++) poly[{F_, j}] = pk.fixed_coeff[j].p;
    for (uint32_t j = 0; j < NUM_SIGMA; j++) poly[{SIGMA_, j}] = pk.sigma_coeff[j].p;
    poly[{PIN_, 0}] = co3[0].p;
    poly[{PTAB_, 0}] = co3[1].p;
    poly[{Z_, 0}] = co3[2].p;
    poly[{Z_, 1}] = co3[3].p;
    poly[{LZ_, 0}] = co3[4].p;
    poly[{RANDOM_, 0}] = random_poly.p;
    point = RotationPoints{x, dom.omega, dom.omega_inv};
    const auto order = eval_order();
    std::vector<void*> ev_polys;
    std::vector<Fr> ev_points;
    for (auto& q : order) {
      ev_polys.push_back(poly.at(q.key));
      ev_points.push_back(point(q.rot));
    }
    for (uint32_t i = 0; i < QUOTIENT_PIECES; i++) {   // the quotient pieces at x ride along: h(x) = sum_i x^(n i) h_i(x)
      ev_polys.push_back(pieces[i]);
      ev_points.push_back(x);
    }
    mark("5: evaluation list built");
    std::vector<Fr> ev(ev_polys.size());
    ck(sg_fr_eval_poly_batch_dev(ev_polys.data(), n, ev_points[0].bytes(), (uint32_t)ev_polys.size(), st.ms,
                                 reinterpret_cast<uint8_t*>(ev.data())), "evaluations");
    mark("5: evaluations back");
    for (size_t i = 0; i < order.size(); i++) {
      evals.at[{order[i].key, order[i].rot}] = ev[i];
      tr.write_scalar(ev[i]);
    }
    evals.h = h_at_x(&ev[order.size()], x_n);
  }

  // -- 6: SHPLONK (the scalars: summa_proof_host.hpp)
  void multiopen() {
    const auto denom_inv = lagrange_denominators_inv(sets, point);
    mark("6: Lagrange denominators inverted");
    const auto zps = zeta_powers(sets, zeta);
    std::vector<std::vector<Fr>> rs;
    for (size_t si = 0; si < sets.size(); si++) rs.push_back(remainder_coefficients(sets[si], zps[si], denom_inv[si], point, evals));
    mark("6: r_i interpolated");
    {
      // f_i = q_i - r_i for all five sets in ONE launch (grid.y = set): q_i = the zeta-combination of the set's polynomials, r_i by value
      const std::vector<Fr> xn_pow = xn_powers(x_n);
      std::vector<void*> ps, outs;
      std::vector<Fr> cs, lows(sets.size() * 4, Fr::zero());
      std::vector<uint32_t> sizes, n_lows;
      for (size_t si = 0; si < sets.size(); si++) {
        const auto& set = sets[si];
        uint32_t count = 0;
        for (size_t j = 0; j < set.polys.size(); j++) {
          if (set.polys[j].kind == H_) {
            for (uint32_t i = 0; i < QUOTIENT_PIECES; i++, count++) {
              ps.push_back(pieces[i]);
              cs.push_back(zps[si][j] * xn_pow[i]);
            }
          } else {
            ps.push_back(poly.at(set.polys[j]));
            cs.push_back(zps[si][j]);
            count++;
          }
        }
        sizes.push_back(count);
        for (size_t t = 0; t < rs[si].size(); t++) lows[4 * si + t] = -rs[si][t];
        n_lows.push_back((uint32_t)rs[si].size());
        fs.emplace_back(n);
        outs.push_back(fs.back().p);
      }
      ck(sg_fr_lincomb_sets_dev(ps.data(), cs[0].bytes(), sizes.data(), (uint32_t)sets.size(), n, lows[0].bytes(), n_lows.data(), outs.data(),
                                st.ms), "set lincombs");
    }
    mark("6: set combinations enqueued");
    // f_i / Z_{S_i} as eleven independent exact Kate divisions (division_weights): ONE batch (three launches for all eleven), and
    // f = sum_i nu^i f_i / Z_{S_i} is one linear combination of the eleven quotients
    f_all = DevCol(n);
    {
      const Divisions div = division_weights(sets, denom_inv, point, nu);
      std::vector<void*> div_in, div_out;
      for (size_t si = 0; si < sets.size(); si++) {
        for (size_t j = 0; j < sets[si].rots.size(); j++) {
          quotients.emplace_back(n);
          div_in.push_back(fs[si].p);
          div_out.push_back(quotients.back().p);
        }
      }
      ck(sg_fr_kate_division_batch_dev(div_in.data(), n, div.points[0].bytes(), (uint32_t)div_in.size(), div_out.data(), st.ms),
         "kate division batch");
      ck(sg_fr_lincomb_dev(div_out.data(), div.weights[0].bytes(), (uint32_t)div_out.size(), n, f_all.p, st.ms), "f lincomb");
    }
    mark("6: f(X) enqueued, commit issued");
    write_points(commit({f_all.p}, {0}), 0, 1);
    mark("6: W back");
    const Fr mu = tr.squeeze();
    const Linearisation lin = linearisation(sets, rs, point, nu, mu);
    std::vector<void*> lp = ptrs(fs);
    lp.push_back(f_all.p);
    l_poly = DevCol(n);
    w2 = DevCol(n);
    ck(sg_fr_lincomb_low_dev(lp.data(), lin.coeffs[0].bytes(), (uint32_t)lp.size(), n, lin.low[0].bytes(), (uint32_t)lin.low.size(), l_poly.p,
                             st.ms), "L lincomb");
    // the remainder L(mu) goes to mapped host memory and is looked at once W' is back: the commitment job is issued behind the
    // division without a host wait in between (a non-zero remainder is a bug in this driver, not an input error)
    std::memset(pinned_small_rows() + 4 * MAIL_REMAINDER, 0xff, 32);   // (not a remainder any kernel writes: a stale zero cannot pass)
    ck(sg_fr_kate_division_rem_dev(l_poly.p, n, mu.bytes(), w2.p, pinned_small_dev_row(MAIL_REMAINDER), st.ms), "final division");
    mark("6: final quotient enqueued, commit issued");
    write_points(commit({w2.p}, {0}), 0, 1);
    mark("6: W' back");
    {
      Fr rem;
      std::memcpy(rem.l, pinned_small_rows() + 4 * MAIL_REMAINDER, 32);
      if (!rem.is_zero()) throw std::runtime_error("multi-open linearisation does not vanish at mu");
    }
  }
};

// advice: 3 device columns (Lagrange, n rows; the last 6 rows are overwritten with blinding values)
template <class Transcript>
std::vector<uint8_t> create_proof_with(const ProvingKey& pk, std::vector<DevCol>& advice, const std::vector<Fr>& instances,
                                       Transcript& tr, const Options& opt = Options(), Timings* timings = nullptr) {
  if (advice.size() != NUM_ADVICE) throw std::invalid_argument("create_proof: three advice columns expected");
  for (auto& a : advice)
    if (a.rows != pk.n || !a.p) throw std::invalid_argument("create_proof: advice columns of 2^k rows expected");
  if (instances.size() > pk.usable) throw std::invalid_argument("create_proof: more instances than usable rows");
  return ProofRun<Transcript>(pk, advice, instances, tr, opt, timings).prove();
}
// the Keccak / EVM flavour (what tools/create_proof_main.cpp and the bundles use)
inline std::vector<uint8_t> create_proof(const ProvingKey& pk, std::vector<DevCol>& advice, const std::vector<Fr>& instances,
                                         Timings* timings = nullptr, const Options& opt = Options()) {
  EvmTranscript tr;
  return create_proof_with(pk, advice, instances, tr, opt, timings);
}

}  // namespace prover
}  // namespace summa
