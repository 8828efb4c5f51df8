// host_threads.h -- the library's own host threads (host_threads.cpp): CPU topology, where the solve's threads are placed,
// the placement monitor, and the one Worker type every thread of the solve runs on.  The jobs and their hand-over protocols
// stay with the Cholesky (block_solver.cpp).
#pragma once
#include <pthread.h>
#include <sched.h>

#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

namespace sage
{
double mono_seconds(); // CLOCK_MONOTONIC in seconds (out of line: keeps the clock out of the target_clones bodies)

// ---- CPU topology (sysfs)
std::vector<int> read_cpu_list(const char *path); // a cpulist file ("0-7,128-135") -> cpu numbers (< CPU_SETSIZE)
std::vector<int> placement_core_siblings(int cpu); // hardware threads of the physical core of `cpu` (at least `cpu`)
std::vector<int> placement_l3_domain(int cpu);     // CPUs that share the L3 of `cpu` (empty: not exposed)
std::vector<int> placement_busy_cpus(int ms);      // CPUs > 25 % busy during `ms` milliseconds (empty: no counters)
// which CPUs the solve's threads may be placed on; nullptr: back to the calling thread's affinity mask
void placement_set_allowed(const cpu_set_t *allowed);
int placement_helper_cpus(int *cpus, int n); // CPUs the solve's (up to three) helper threads are pinned to
int placement_monitor_moves();              // threads moved off crowded cores so far (placement monitor)

// One kind of thread of the solve: `n` threads that share one job (a Cholesky helper: n = 1; the arrow-row pool: n =
// SAGE_SOLVE_POOL).  They sleep on a condition variable until the worker is armed, then spin: every change of `posted` runs
// run(t) once on each thread t.  After `idle_s` seconds without a post they disarm the worker and sleep again -- unless
// hold() says a client still counts on them.  The objects live for the life of the process; their threads come and go
// (start: block_chol_arm, stop and join: host_threads_shutdown).
struct Worker
{
  explicit Worker(int n_threads, double idle) : n(n_threads), idle_s(idle), th(new Thread[n_threads]) {}
  virtual ~Worker() = default;
  virtual void run(int t) = 0;
  virtual bool hold() const { return false; }

  const int n;
  const double idle_s;
  std::atomic<bool> armed{false};
  std::atomic<unsigned> posted{0};
  std::atomic<int> near_cpu{-1}, near_mode{-1}; // the caller's CPU and mode it was placed for (-1: not placed)
  struct Thread
  {
    std::thread th;
    pthread_t tid{};
    std::atomic<int> ktid{0}; // kernel thread id (its /proc/self/task entry: the placement monitor reads its run-queue delay)
    std::atomic<int> cpu{-1}; // the CPU it is pinned to (-1: not pinned)
    std::atomic<int> dom{0};  // pool: 0 / 1 = on the first / second half's L3 domain, -1 elsewhere (place_pool)
  };
  const std::unique_ptr<Thread[]> th;
  std::atomic<bool> running{false};

  void arm();   // wake the threads (they spin for a post)
  void start(); // (g_threads_mu held; no-op when running)
  void stop();  // quit and join (g_threads_mu held, solve lease held exclusively)

private:
  void loop(int t);
  std::mutex mu;
  std::condition_variable cv;
  std::atomic<bool> quit{false};
  unsigned seen0 = 0;
};

// the solve's workers (block_solver.cpp): 0 = the second half's helper, 1 / 2 = the look-ahead stages of the halves (null on
// hosts with too few CPUs), 3 = the arrow-row pool (null: none; only made when `make`)
constexpr int kSolveWorkers = 4;
Worker *solve_worker(int idx, bool make = true);

// Every arm-then-solve sequence holds a solve lease (shared) from before block_chol_arm until block_chol_solve_tr has
// returned; host_threads_shutdown takes it exclusively, so no thread is joined while a solve can pin, arm, post to or wait
// on it.  A lease does not nest (writers are preferred: a second shared lease behind a waiting shutdown would deadlock).
struct SolveLease
{
  explicit SolveLease(bool exclusive = false);
  ~SolveLease();
  SolveLease(const SolveLease &) = delete;
  SolveLease &operator=(const SolveLease &) = delete;
};

// Wake the helper threads ahead of a block_chol_solve_tr call with n1 > 0 (they then spin for the job for a few
// milliseconds at most); call it when the system is about to be produced, e.g. before waiting on the D2H copy, with a
// SolveLease held.  with_pool: also wake the worker pool that shares the long separator ("arrow") rows of a loop-closure
// plan.  Returns true when the solve should run its halves without look-ahead stages (BlockEnvelope::no_lookahead): a plan
// whose long arrow-row chains (block_plan_long_arrow_chains) do not fit the cores the look-ahead stages leave free in the
// caller's L3 domain but do fit with those two cores.
bool block_chol_arm(bool with_pool = false, int long_arrow_chains = 0);
// the arrow-row pool's placement, read by block_solver.cpp's task split: pool workers per L3 domain (-1: unknown / no pool),
// and whether the second half, its look-ahead stage and its chains sit on a domain of their own
extern std::atomic<int> g_domain_threads[2];
extern std::atomic<bool> g_two_domains;

// r06: the placement monitor is OPT-IN (SAGE_PLACEMENT_MONITOR=1 or placement_monitor_enable(1)); every thread the solve
// starts (helpers, arrow-row pool, monitor) is joinable: host_threads_shutdown() waits for the solves in flight, stops and
// joins them (the monitor first); the next block_chol_arm() starts them again.  host_threads_running() = how many are alive.
void placement_monitor_enable(int on);
int placement_monitor_running();
void host_threads_shutdown();
int host_threads_running();
} // namespace sage
