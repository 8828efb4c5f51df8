// host_threads.cpp -- the library's own host threads: CPU topology, where the solve's threads are placed, pinning, the
// placement monitor, and the life cycle of every thread the library starts (host_threads.h).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <map>
#include <sys/syscall.h>
#include <unistd.h>

#include "host_math.h" // env_flag
#include "host_threads.h"

namespace sage
{
double mono_seconds()
{
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

// ---- CPU topology
std::vector<int> read_cpu_list(const char *path)
{
  std::vector<int> out;
  FILE *f = fopen(path, "r");
  if (!f)
    return out;
  char buf[4096];
  if (fgets(buf, sizeof(buf), f))
    for (const char *p = buf; *p;)
    {
      char *end;
      const long a = strtol(p, &end, 10);
      if (end == p)
        break;
      long b = a;
      p = end;
      if (*p == '-')
      {
        b = strtol(p + 1, &end, 10);
        p = end;
      }
      for (long c = a; c <= b && c < CPU_SETSIZE; ++c)
        out.push_back((int)c);
      if (*p == ',')
        ++p;
    }
  fclose(f);
  return out;
}

std::vector<int> placement_core_siblings(int cpu)
{
  char path[128];
  snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list", cpu);
  std::vector<int> sib = read_cpu_list(path);
  if (sib.empty())
    sib.push_back(cpu);
  return sib;
}

std::vector<int> placement_l3_domain(int cpu)
{
  char path[128];
  snprintf(path, sizeof(path), "/sys/devices/system/cpu/cpu%d/cache/index3/shared_cpu_list", cpu);
  return read_cpu_list(path);
}

static std::vector<int> node_cpus_of(int cpu)
{
  char path[128];
  for (int node = 0; node < 64; ++node)
  {
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    const std::vector<int> nl = read_cpu_list(path);
    if (std::find(nl.begin(), nl.end(), cpu) != nl.end())
      return nl;
  }
  return {};
}

// per CPU: (all ticks, idle + iowait ticks) since boot
using CpuTimes = std::map<int, std::pair<unsigned long long, unsigned long long>>;
static bool stat_snapshot(CpuTimes &m)
{
  FILE *f = fopen("/proc/stat", "r");
  if (!f)
    return false;
  char line[512];
  while (fgets(line, sizeof(line), f))
  {
    int cpu;
    unsigned long long v[8] = {0};
    if (sscanf(line, "cpu%d %llu %llu %llu %llu %llu %llu %llu %llu", &cpu, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6],
               &v[7]) >= 5)
    {
      unsigned long long tot = 0;
      for (int i = 0; i < 8; ++i)
        tot += v[i];
      m[cpu] = {tot, v[3] + v[4]};
    }
  }
  fclose(f);
  return !m.empty();
}
// non-idle share of CPU `c` between two snapshots (0 when either misses it or the window has < 4 USER_HZ ticks)
static double cpu_load(const CpuTimes &a, const CpuTimes &b, int c)
{
  auto x = a.find(c), y = b.find(c);
  if (x == a.end() || y == b.end())
    return 0.0;
  const double tot = (double)(y->second.first - x->second.first), idle = (double)(y->second.second - x->second.second);
  return tot >= 4.0 ? 1.0 - idle / tot : 0.0;
}

std::vector<int> placement_busy_cpus(int ms)
{
  CpuTimes a, b;
  std::vector<int> out;
  if (!stat_snapshot(a))
    return out;
  std::this_thread::sleep_for(std::chrono::milliseconds(ms));
  if (!stat_snapshot(b))
    return out;
  for (const auto &kv : a)
    if (cpu_load(a, b, kv.first) > 0.25)
      out.push_back(kv.first);
  return out;
}

// ---- which CPUs the solve's threads may be placed on.  Default: the calling thread's affinity mask.  r05: a GPU box is a
// slice of a node whose other GPUs run other jobs -- their host threads sit on CPUs of the same NUMA node, and a helper
// pinned onto a core another tenant saturates runs its half of the factorisation at half speed for the life of the
// process (~1 process in 8 measured +60..200 us per solve).  sage_bind_thread_to_device therefore samples the CPU load and
// hands over the CPUs of QUIET physical cores (placement_set_allowed); the caller's own mask may be narrower than that
// (its L3 domain), the loop-closure plans' second domain is looked for in the handed-over set.
static std::mutex g_place_mu;
static bool g_place_override = false;
static cpu_set_t g_place_allowed;
// (heap-allocated and never destroyed: a thread of this library may still look at them while the process runs its static
//  destructors)
static std::map<std::pair<int, bool>, std::vector<int>> &g_ccx_cache = *new std::map<std::pair<int, bool>, std::vector<int>>;
static std::map<std::pair<int, size_t>, std::vector<int>> &g_dom2_cache = *new std::map<std::pair<int, size_t>, std::vector<int>>;

void placement_set_allowed(const cpu_set_t *allowed)
{
  std::lock_guard<std::mutex> lk(g_place_mu);
  g_place_override = allowed != nullptr;
  if (allowed)
    g_place_allowed = *allowed;
  g_ccx_cache.clear();
  g_dom2_cache.clear();
}

static bool placement_allowed(cpu_set_t *out) // (g_place_mu held)
{
  if (g_place_override)
  {
    *out = g_place_allowed;
    return true;
  }
  return sched_getaffinity(0, sizeof(*out), out) == 0;
}

// Thread placement of the solve: the caller, the helper of the second half and the worker pool each get their own
// PHYSICAL core of the caller's CCX (cores that share its L3): the halves and the arrow-row tasks then work out of one
// cache and one NUMA node (a helper on the far socket takes ~35 % longer for its half), and no two of them share a core
// through SMT (r03: a pool thread on the helper's sibling made the helper's half 35-45 % slower on config 5).
// cores[0] -> helper, cores[1 + t] -> pool thread t; threads the CCX has no core left for fall back to the rest of the
// caller's NUMA node as a set.
static std::vector<int> sibling_free_cores(const std::vector<int> &cpus, int caller_cpu, const cpu_set_t &allowed)
{
  auto core_of = [](int c) {
    const std::vector<int> sib = placement_core_siblings(c);
    return *std::min_element(sib.begin(), sib.end());
  };
  const int caller_core = core_of(caller_cpu);
  std::vector<int> cores, seen_core;
  for (int c : cpus)
  {
    if (c >= CPU_SETSIZE || !CPU_ISSET(c, &allowed))
      continue;
    const int core = core_of(c);
    if (core == caller_core || std::find(seen_core.begin(), seen_core.end(), core) != seen_core.end())
      continue;
    seen_core.push_back(core);
    cores.push_back(c); // the first allowed hardware thread of that core
  }
  return cores;
}

// (sysfs is read once per caller CPU: the arm call sits at the start of every solve; returned by value -- the cache is
//  cleared when the allowed set changes)
static std::vector<int> ccx_cores_of(int cpu, bool with_node)
{
  std::lock_guard<std::mutex> lk(g_place_mu);
  auto it = g_ccx_cache.find({cpu, with_node});
  if (it != g_ccx_cache.end())
    return it->second;
  std::vector<int> cores;
  const std::vector<int> l3 = placement_l3_domain(cpu);
  cpu_set_t allowed;
  if (!l3.empty() && placement_allowed(&allowed))
  {
    cores = sibling_free_cores(l3, cpu, allowed);
    if (with_node)
      for (int c : sibling_free_cores(node_cpus_of(cpu), cpu, allowed))
        if (std::find(cores.begin(), cores.end(), c) == cores.end())
          cores.push_back(c);
  }
  return g_ccx_cache.emplace(std::make_pair(cpu, with_node), std::move(cores)).first->second;
}

// cores of ANOTHER L3 domain of the caller's NUMA node (the next one with at least `want` free physical cores), or empty
// (sysfs is read once per caller CPU and size: the arm call sits at the start of every solve)
static std::vector<int> second_domain_cores(int cpu, size_t want)
{
  std::lock_guard<std::mutex> lk(g_place_mu);
  auto it = g_dom2_cache.find({cpu, want});
  if (it != g_dom2_cache.end())
    return it->second;
  std::vector<int> &out = g_dom2_cache[{cpu, want}];
  const std::vector<int> l3a = placement_l3_domain(cpu);
  cpu_set_t allowed;
  if (l3a.empty() || !placement_allowed(&allowed))
    return out;
  std::vector<int> seen = l3a;
  for (int c : node_cpus_of(cpu))
  {
    if (std::find(seen.begin(), seen.end(), c) != seen.end() || c >= CPU_SETSIZE || !CPU_ISSET(c, &allowed))
      continue;
    const std::vector<int> l3b = placement_l3_domain(c);
    if (l3b.empty())
      continue;
    seen.insert(seen.end(), l3b.begin(), l3b.end());
    std::vector<int> cores = sibling_free_cores(l3b, cpu, allowed);
    if (cores.size() >= want)
      return out = std::move(cores);
  }
  return out;
}

// the placement code and the placement monitor pin under this lock: a thread's recorded cpu and its affinity stay in step
static std::mutex g_pin_mu;
static void pin_one(pthread_t t, int cpu)
{
  cpu_set_t want;
  CPU_ZERO(&want);
  CPU_SET(cpu, &want);
  (void)pthread_setaffinity_np(t, sizeof(want), &want);
}

// ---- life cycle.  One owner: every start and every join is decided under g_threads_mu, and a join also holds the solve
// lease exclusively -- so no solve is between its arm and the end of its block_chol_solve_tr (where it may pin, arm, post
// to or wait on any worker, also one another caller armed).  Lock order: lease, g_threads_mu, the rest.
static pthread_rwlock_t g_solve_lease = PTHREAD_RWLOCK_WRITER_NONRECURSIVE_INITIALIZER_NP;
SolveLease::SolveLease(bool exclusive)
{
  (void)(exclusive ? pthread_rwlock_wrlock(&g_solve_lease) : pthread_rwlock_rdlock(&g_solve_lease));
}
SolveLease::~SolveLease() { (void)pthread_rwlock_unlock(&g_solve_lease); }

static std::mutex g_threads_mu;
static void host_threads_atexit_once()
{
  static std::once_flag once;
  std::call_once(once, [] { atexit(host_threads_shutdown); });
}

void Worker::arm()
{
  {
    std::lock_guard<std::mutex> lk(mu);
    armed.store(true, std::memory_order_release);
  }
  cv.notify_all();
}

void Worker::start()
{
  if (running.load(std::memory_order_acquire))
    return;
  host_threads_atexit_once();
  quit.store(false, std::memory_order_release);
  near_cpu.store(-1, std::memory_order_release); // new threads: not pinned yet, the next arm places them again
  near_mode.store(-1, std::memory_order_release);
  seen0 = posted.load(std::memory_order_acquire);
  for (int t = 0; t < n; ++t)
  {
    th[t].ktid.store(0, std::memory_order_release);
    th[t].cpu.store(-1, std::memory_order_release);
    th[t].th = std::thread([this, t] {
      th[t].ktid.store((int)syscall(SYS_gettid), std::memory_order_release);
      loop(t);
    });
    th[t].tid = th[t].th.native_handle();
  }
  running.store(true, std::memory_order_release);
}

void Worker::stop()
{
  if (!running.load(std::memory_order_acquire))
    return;
  {
    std::lock_guard<std::mutex> lk(mu);
    quit.store(true, std::memory_order_release);
  }
  cv.notify_all();
  for (int t = 0; t < n; ++t)
  {
    th[t].th.join();
    th[t].cpu.store(-1, std::memory_order_release);
  }
  armed.store(false, std::memory_order_release);
  running.store(false, std::memory_order_release);
}

void Worker::loop(int t)
{
  unsigned seen = seen0; // (sampled by the thread that started this one, before it can post: a restarted thread does not
                         //  answer posts from before its time and cannot miss the starter's first one)
  for (;;)
  {
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return armed.load(std::memory_order_acquire) || quit.load(std::memory_order_acquire); });
    }
    if (quit.load(std::memory_order_acquire))
      return;
    double t0 = mono_seconds();
    unsigned spins = 0;
    while (armed.load(std::memory_order_acquire) && !quit.load(std::memory_order_relaxed))
    {
      const unsigned p = posted.load(std::memory_order_acquire);
      if (p != seen)
      {
        seen = p;
        run(t);
        t0 = mono_seconds(); // the idle time-out counts from the last post, not from the wake-up
      }
      __builtin_ia32_pause();
      // nobody came: back to sleep.  Not while a client holds the worker (the pool's owner clears `armed` itself when its
      // solve is done: a worker that timed out in the middle of another caller's arm / post must not disarm the pool)
      if ((++spins & 1023) == 0 && mono_seconds() - t0 > idle_s && !hold())
        armed.store(false, std::memory_order_release);
    }
  }
}

static void start_worker(Worker *w)
{
  if (w->running.load(std::memory_order_acquire))
    return;
  std::lock_guard<std::mutex> lk(g_threads_mu);
  w->start();
}

// ---- placement monitor (r05).  The box's other tenants move: a core that was quiet when the helpers were placed may carry
// somebody else's thread a minute later, and a helper that shares its hardware thread (it then waits on the run queue when the
// solve wakes it) or its physical core (SMT: ~2/3 speed) slows every solve of the process from then on.  A background thread
// looks every 250 ms at (a) the run-queue delay of every thread of the solve's workers (their schedstat) and (b) the load on
// the OTHER hardware threads of their cores (stat_snapshot); a thread that is crowded in two consecutive looks is moved to a
// core of its own L3 domain (else the caller's, else the NUMA node) that is idle on all its hardware threads.  r06: OPT-IN
// (SAGE_PLACEMENT_MONITOR=1 or sage_placement_monitor(1)) -- a drop-in library does not edit thread affinities from a
// background thread unless asked to.  SAGE_DEBUG_TIMING prints the moves.
static std::atomic<int> g_monitor_wanted{-1}; // -1: ask the environment, 0 / 1: set through the API
static std::atomic<int> g_monitor_moves{0};
static std::thread &g_monitor = *new std::thread; // (g_threads_mu)
static std::atomic<bool> g_monitor_running{false}; // (written under g_threads_mu)
static std::mutex g_monitor_mu;
static std::condition_variable g_monitor_cv;
static bool g_monitor_stop = false; // (g_monitor_mu)

static long long read_run_delay_ns(int ktid)
{
  char path[96];
  snprintf(path, sizeof(path), "/proc/self/task/%d/schedstat", ktid);
  FILE *f = fopen(path, "r");
  if (!f)
    return -1;
  unsigned long long run = 0, delay = 0;
  const int n = fscanf(f, "%llu %llu", &run, &delay);
  fclose(f);
  return n == 2 ? (long long)delay : -1;
}

static void placement_monitor_loop()
{
  const bool verbose = env_flag("SAGE_DEBUG_TIMING");
  CpuTimes prev, cur;
  // watched threads: every thread of every worker made so far, the helpers' first (the pool comes last, once a loop-closure
  // plan has made it -- so a thread keeps its slot)
  struct Slot
  {
    Worker *w;
    int worker, t;
  };
  std::vector<Slot> slots;
  std::vector<long long> prev_delay;
  std::vector<int> strikes;
  stat_snapshot(prev);
  {
    // its own affinity: the CPUs the placement may use (not the one-L3 mask inherited from the LM thread that started it,
    // where it would compete with the thread that spins)
    cpu_set_t allowed;
    bool ok;
    {
      std::lock_guard<std::mutex> lk(g_place_mu);
      ok = placement_allowed(&allowed);
    }
    if (ok)
      (void)pthread_setaffinity_np(pthread_self(), sizeof(allowed), &allowed);
  }
  for (;;)
  {
    {
      std::unique_lock<std::mutex> lm(g_monitor_mu);
      if (g_monitor_cv.wait_for(lm, std::chrono::milliseconds(250), [] { return g_monitor_stop; }))
        return;
    }
    cur.clear();
    if (!stat_snapshot(cur))
      continue;
    auto busy = [&](int c) { return cpu_load(prev, cur, c); };
    slots.clear();
    for (int i = 0; i < kSolveWorkers; ++i)
      if (Worker *w = solve_worker(i, false))
        for (int t = 0; t < w->n; ++t)
          slots.push_back({w, i, t});
    prev_delay.resize(slots.size(), -1);
    strikes.resize(slots.size(), 0);
    // (a worker's threads are joined only after this thread: a running worker's tid stays valid while it looks)
    auto live_cpu = [](const Slot &s) {
      return s.w->running.load(std::memory_order_acquire) ? s.w->th[s.t].cpu.load(std::memory_order_acquire) : -1;
    };
    Worker *h0 = solve_worker(0, false), *q = solve_worker(kSolveWorkers - 1, false);
    const int near = h0 ? h0->near_cpu.load(std::memory_order_acquire) : (q ? q->near_cpu.load(std::memory_order_acquire) : -1);
    for (size_t i = 0; i < slots.size(); ++i)
    {
      const Slot &s = slots[i];
      Worker::Thread &x = s.w->th[s.t];
      const int c = live_cpu(s), kt = x.ktid.load(std::memory_order_acquire);
      if (c < 0 || kt <= 0)
        continue;
      const long long d = read_run_delay_ns(kt);
      const long long dd = (d >= 0 && prev_delay[i] >= 0) ? d - prev_delay[i] : 0;
      prev_delay[i] = d;
      bool crowded = dd > 2000000; // > 2 ms on the run queue in a quarter second: somebody shares the hardware thread
      double sib_busy = 0.0;
      for (int sib : placement_core_siblings(c))
        if (sib != c)
          sib_busy = std::max(sib_busy, busy(sib));
      crowded = crowded || sib_busy > 0.3;
      strikes[i] = crowded ? strikes[i] + 1 : 0;
      if (strikes[i] < 2 || near < 0)
        continue;
      // a quiet core: the thread's own L3 domain first (a pool worker of the second half's domain stays there), then the
      // caller's domain and node; idle on all hardware threads, not used by another watched thread
      std::vector<int> cands = placement_l3_domain(c);
      for (int y : ccx_cores_of(near, true))
        cands.push_back(y);
      cpu_set_t allowed;
      {
        std::lock_guard<std::mutex> lk(g_place_mu);
        if (!placement_allowed(&allowed))
          continue;
      }
      const std::vector<int> near_sib = placement_core_siblings(near);
      int target = -1;
      for (int cand : cands)
      {
        if (cand >= CPU_SETSIZE || !CPU_ISSET(cand, &allowed) || std::find(near_sib.begin(), near_sib.end(), cand) != near_sib.end())
          continue;
        bool ok = true;
        for (int sib : placement_core_siblings(cand))
        {
          ok = ok && busy(sib) < 0.1;
          for (size_t j = 0; j < slots.size() && ok; ++j)
            ok = live_cpu(slots[j]) != sib;
        }
        if (ok)
        {
          target = cand;
          break;
        }
      }
      if (target < 0)
        continue;
      {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        pin_one(x.tid, target);
        x.cpu.store(target, std::memory_order_release);
      }
      g_monitor_moves.fetch_add(1, std::memory_order_relaxed);
      strikes[i] = 0;
      if (verbose)
        fprintf(stderr, "[sage placement] %s %d: cpu %d crowded (run-queue delay %.1f ms, sibling load %.0f %%) -> cpu %d\n",
                s.worker < 3 ? "helper" : "pool worker", s.worker < 3 ? s.worker : s.t, c, dd * 1e-6, 100.0 * sib_busy, target);
    }
    prev.swap(cur);
  }
}

static bool placement_monitor_wanted()
{
  int want = g_monitor_wanted.load(std::memory_order_acquire);
  if (want < 0)
  {
    const char *e = getenv("SAGE_PLACEMENT_MONITOR");
    want = (e && atoi(e) != 0) ? 1 : 0;
    g_monitor_wanted.store(want, std::memory_order_release);
  }
  return want != 0;
}
// (g_threads_mu held)
static void placement_monitor_start()
{
  if (g_monitor.joinable() || !placement_monitor_wanted())
    return;
  host_threads_atexit_once();
  {
    std::lock_guard<std::mutex> lm(g_monitor_mu);
    g_monitor_stop = false;
  }
  g_monitor = std::thread(placement_monitor_loop);
  g_monitor_running.store(true, std::memory_order_release);
}
// (g_threads_mu held)
static void placement_monitor_stop()
{
  if (!g_monitor.joinable())
    return;
  {
    std::lock_guard<std::mutex> lm(g_monitor_mu);
    g_monitor_stop = true;
  }
  g_monitor_cv.notify_all();
  g_monitor.join();
  g_monitor_running.store(false, std::memory_order_release);
}
void placement_monitor_enable(int on)
{
  g_monitor_wanted.store(on ? 1 : 0, std::memory_order_release);
  if (!on)
  {
    std::lock_guard<std::mutex> lk(g_threads_mu);
    placement_monitor_stop();
  }
}
int placement_monitor_running() { return g_monitor_running.load(std::memory_order_acquire) ? 1 : 0; }
int placement_monitor_moves() { return g_monitor_moves.load(std::memory_order_relaxed); }

int placement_helper_cpus(int *cpus, int n)
{
  int k = 0;
  for (int idx = 0; idx < 3 && k < n; ++idx)
    if (Worker *h = solve_worker(idx))
      cpus[k++] = h->th[0].cpu.load(std::memory_order_acquire);
  return k;
}

// ---- placement of the solve's workers.
// mode 0: everything on the caller's L3 domain A -- A[0] second half, A[1] / A[2] look-ahead stages, pool from A[3] on;
// mode 1: no look-ahead stages -- A[0] second half, pool from A[1] on;
// mode 2 (two domains): A[0] look-ahead of the first half, pool workers for the first half's chains from A[1] on;
//         B[0] second half, B[1] its look-ahead stage, pool workers for the second half's chains from B[2] on
std::atomic<int> g_domain_threads[2] = {{-1}, {0}};
std::atomic<bool> g_two_domains{false};

// a worker is placed again only when the caller's CPU or the mode changed since it was last placed
static bool place_once(Worker *w, int cpu, int mode)
{
  if (cpu < 0 || (cpu == w->near_cpu.load(std::memory_order_acquire) && mode == w->near_mode.load(std::memory_order_acquire)))
    return false;
  w->near_cpu.store(cpu, std::memory_order_release);
  w->near_mode.store(mode, std::memory_order_release);
  return true;
}

static void place_helper(Worker *h, int cpu, int idx, int mode, const std::vector<int> &B)
{
  if (!place_once(h, cpu, mode))
    return;
  const std::vector<int> &A = ccx_cores_of(cpu, false);
  int core = -1;
  if (mode == 2)
    core = idx == 0 ? (B.size() > 0 ? B[0] : -1) : idx == 1 ? (A.size() > 0 ? A[0] : -1) : (B.size() > 1 ? B[1] : -1);
  else if ((int)A.size() > idx)
    core = A[idx];
  if (core >= 0)
  {
    std::lock_guard<std::mutex> pin_lk(g_pin_mu);
    pin_one(h->th[0].tid, core);
    h->th[0].cpu.store(core, std::memory_order_release);
  }
}

static void place_pool(Worker *q, int cpu, int mode, const std::vector<int> &B, int chains_per_half)
{
  if (!place_once(q, cpu, mode))
    return;
  const std::vector<int> &cores = ccx_cores_of(cpu, true); // domain A first, then the rest of the NUMA node
  const size_t n_ccx = ccx_cores_of(cpu, false).size();
  const size_t nq = (size_t)q->n;
  std::lock_guard<std::mutex> pin_lk(g_pin_mu);
  auto pin = [&](size_t t, int core, int dom) {
    pin_one(q->th[t].tid, core);
    q->th[t].cpu.store(core, std::memory_order_release);
    q->th[t].dom.store(dom, std::memory_order_release);
  };
  for (size_t t = 0; t < nq; ++t)
    q->th[t].dom.store(-1, std::memory_order_release);
  int n0 = 0, n1 = 0;
  if (mode == 2)
  {
    size_t t = 0;
    for (size_t c = 1; c < n_ccx && (int)c <= chains_per_half && t < nq; ++c, ++t, ++n0)
      pin(t, cores[c], 0);
    for (size_t c = 2; c < B.size() && (int)c - 1 <= chains_per_half && t < nq; ++c, ++t, ++n1)
      pin(t, B[c], 1);
    // the rest: the remaining cores of domain A, then of the node (short tasks, pair products, back substitution)
    for (size_t c = 1 + (size_t)n0; t < nq && c < cores.size(); ++c)
      if (std::find(B.begin(), B.end(), cores[c]) == B.end())
        pin(t++, cores[c], -1);
  }
  else
  {
    const size_t off = mode == 1 ? 1 : 3;
    for (size_t t = 0; t < nq && t + off < cores.size(); ++t)
    {
      pin(t, cores[t + off], t + off < n_ccx ? 0 : -1);
      n0 += t + off < n_ccx ? 1 : 0;
    }
  }
  g_domain_threads[0].store(n0, std::memory_order_release);
  g_domain_threads[1].store(n1, std::memory_order_release);
  g_two_domains.store(mode == 2, std::memory_order_release);
}

bool block_chol_arm(bool with_pool, int long_arrow_chains)
{
  static const bool no_la_env = env_flag("SAGE_SOLVE_NO_LOOKAHEAD");
  const int cpu = sched_getcpu();
  // r05: a loop-closure plan's long arrow-row chains run ~30 % slower on another L3 domain than their half and the separator
  // then waits for them (config 5: six chains, four cores left next to the two halves and their look-ahead stages: 1.1-1.4 ms).
  // The two halves do not reference each other: when the chains do not fit domain A, the SECOND half moves to a domain B of
  // its own with its look-ahead stage and its chains (mode 2) -- every chain then sits next to the half it follows.  Without
  // a second domain the look-ahead stages' cores go to the chains when that makes them fit (mode 1).
  int mode = no_la_env ? 1 : 0;
  std::vector<int> B;
  const int per_half = (long_arrow_chains + 1) / 2;
  if (mode == 0 && with_pool && long_arrow_chains > 0 && !env_flag("SAGE_SOLVE_KEEP_LOOKAHEAD"))
  {
    const int n_ccx = (int)ccx_cores_of(cpu, false).size(); // cores of domain A without the caller's
    if (long_arrow_chains > n_ccx - 3)
    {
      if (!env_flag("SAGE_SOLVE_ONE_DOMAIN"))
        B = second_domain_cores(cpu, (size_t)(2 + per_half));
      if (!B.empty() && n_ccx >= 1 + per_half)
        mode = 2;
      else if (long_arrow_chains <= n_ccx - 1)
        mode = 1;
    }
  }
  const bool no_la = mode == 1;
  for (int idx = 0; idx < (no_la ? 1 : 3); ++idx)
  {
    Worker *h = solve_worker(idx);
    if (!h)
      continue;
    start_worker(h);
    if (!h->armed.load(std::memory_order_acquire))
    {
      place_helper(h, cpu, idx, mode, B);
      h->arm();
    }
  }
  if (placement_monitor_wanted() && !g_monitor_running.load(std::memory_order_acquire))
  {
    std::lock_guard<std::mutex> lk(g_threads_mu);
    placement_monitor_start();
  }
  Worker *q = with_pool ? solve_worker(kSolveWorkers - 1) : nullptr;
  if (q)
  {
    start_worker(q);
    if (!q->armed.load(std::memory_order_acquire))
    {
      place_pool(q, cpu, mode, B, per_half);
      q->arm();
    }
  }
  return no_la;
}

// Stop and join every host thread this library started: the placement monitor first (it pins the others), then the
// workers.  Waits for the solves in flight; the next block_chol_arm() starts the threads again.  Called by sage_shutdown(),
// by the last sage_window_destroy and at process exit.
void host_threads_shutdown()
{
  SolveLease lease(true);
  std::lock_guard<std::mutex> lk(g_threads_mu);
  placement_monitor_stop();
  for (int i = 0; i < kSolveWorkers; ++i)
    if (Worker *w = solve_worker(i, false))
      w->stop();
}

int host_threads_running()
{
  int n = placement_monitor_running();
  for (int i = 0; i < kSolveWorkers; ++i)
    if (Worker *w = solve_worker(i, false))
      n += w->running.load(std::memory_order_acquire) ? w->n : 0;
  return n;
}
} // namespace sage
