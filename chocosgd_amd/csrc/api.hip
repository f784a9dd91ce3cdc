// Library-wide C-ABI plumbing: per-thread error text, version, profiling hooks.
#include "choco_common.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace choco {

static thread_local char g_err[1024] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(CHOCO_ERR_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
  return CHOCO_OK;
}

// ---------------------------------------------------------------- profiling
struct PendingEv {
  const char* name;
  hipEvent_t a, b;
};
static std::atomic<bool> g_prof_on{false};
static std::mutex g_prof_mu;
static std::vector<PendingEv> g_pending;   // pairs a launch has recorded, not yet read
static std::map<std::string, std::pair<double, int64_t>> g_acc;
static std::vector<std::string> g_filter;  // only these kernel names are timed (empty = all)
static std::vector<hipEvent_t> g_free_ev;  // events are reused: no create/destroy per launch

// the named call sites (choco_launch_count: the bench's warm-hit rates); a site registers
// once, when its first launch constructs it, and lives as long as the library
static std::mutex g_sites_mu;
static std::vector<const LaunchSite*>& sites() {
  static std::vector<const LaunchSite*> v;
  return v;
}

LaunchSite::LaunchSite(const char* name) : name_(name) {
  if (!name) return;
  std::lock_guard<std::mutex> g(g_sites_mu);
  sites().push_back(this);
}

EventPair LaunchSite::begin() {
  EventPair ev{nullptr, nullptr};
  if (!name_) return ev;
  count_.fetch_add(1, std::memory_order_relaxed);
  if (!g_prof_on.load(std::memory_order_relaxed)) return ev;
  std::lock_guard<std::mutex> g(g_prof_mu);
  if (!g_filter.empty() && std::find(g_filter.begin(), g_filter.end(), std::string(name_)) == g_filter.end())
    return ev;
  for (hipEvent_t* e : {&ev.a, &ev.b}) {
    if (!g_free_ev.empty()) {
      *e = g_free_ev.back();
      g_free_ev.pop_back();
    } else if (hipEventCreate(e) != hipSuccess) {
      if (ev.a) g_free_ev.push_back(ev.a);
      return EventPair{nullptr, nullptr};
    }
  }
  return ev;
}

// the launch has recorded this pair: only now may it be read (events are reused)
void LaunchSite::timed(EventPair ev) {
  std::lock_guard<std::mutex> g(g_prof_mu);
  g_pending.push_back(PendingEv{name_, ev.a, ev.b});
}

static void profile_drain_locked() {
  for (auto& p : g_pending) {
    float ms = 0.f;
    if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      auto& e = g_acc[p.name];
      e.first += ms;
      e.second += 1;
    }
    g_free_ev.push_back(p.a);
    g_free_ev.push_back(p.b);
  }
  g_pending.clear();
}

}  // namespace choco

using namespace choco;

CHOCO_API int choco_version(void) { return 1; }

CHOCO_API int choco_last_error(char* buf, size_t len) {
  size_t n = strlen(g_err);
  if (buf && len) {
    size_t c = n < len - 1 ? n : len - 1;
    memcpy(buf, g_err, c);
    buf[c] = 0;
  }
  return (int)n;
}

CHOCO_API int choco_profile_enable(int32_t on) {
  g_prof_on.store(on != 0);
  return CHOCO_OK;
}

CHOCO_API int choco_profile_filter(const char* names) {
  std::lock_guard<std::mutex> g(g_prof_mu);
  g_filter.clear();
  std::string all = names ? names : "";
  size_t p = 0;
  while (p <= all.size()) {
    const size_t q = std::min(all.find(',', p), all.size());
    if (q > p) g_filter.push_back(all.substr(p, q - p));
    p = q + 1;
  }
  return CHOCO_OK;
}

CHOCO_API int choco_profile_read(const char* name, double* total_ms, int64_t* count) {
  std::lock_guard<std::mutex> g(g_prof_mu);
  profile_drain_locked();
  auto it = g_acc.find(name ? name : "");
  if (total_ms) *total_ms = it == g_acc.end() ? 0.0 : it->second.first;
  if (count) *count = it == g_acc.end() ? 0 : it->second.second;
  return CHOCO_OK;
}

CHOCO_API int64_t choco_launch_count(const char* name) {
  std::lock_guard<std::mutex> g(g_sites_mu);
  int64_t n = 0;
  for (const LaunchSite* s : sites())
    if (name && strcmp(s->name(), name) == 0) n += s->count();
  return n;
}

CHOCO_API int choco_profile_reset(void) {
  std::lock_guard<std::mutex> g(g_prof_mu);
  profile_drain_locked();
  g_acc.clear();
  return CHOCO_OK;
}
