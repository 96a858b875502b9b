// The refusals of the host-form schedule entry points, as a stand-alone program for a sanitizer
// build of the host code (make host-refusals): every call below is refused before any GPU call,
// so no device is needed.  Prints each code and message and exits 1 if one is not as expected.
//
// The order under test: a schedule call reports its descriptor's fault with or without a
// handle, then the missing handle; ryd_run_batch and ryd_run_coherences report the handle first.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/ryd_engine.h"

static int bad = 0;

static void expect(const char* what, int rc, int want, const char* msg) {
  const bool ok = rc == want && std::strstr(ryd_last_error(), msg) != nullptr;
  std::printf("%-46s rc = %2d  \"%s\"%s\n", what, rc, ryd_last_error(), ok ? "" : "   <-- UNEXPECTED");
  if (!ok) bad = 1;
}

int main() {
  const int64_t n = 3;
  const int nseg = 5;
  std::vector<double> p(RYD_NPARAM * n, 1.0), tab(n * RYD_SC_NFIELD * nseg, 0.5), st(36 * 4 * n), sm(RYD_NSUMMARY * n),
      jac(n * 4 * RYD_SC_NFIELD * nseg), coh(RYD_NCOH * n);
  std::vector<uint32_t> status(n);
  ryd_stats stats;
  ryd_sched_desc good = {};
  good.abi_version = RYD_ABI_VERSION;
  good.dim = 3;
  good.n_seg = nseg;
  good.flags = RYD_FLAG_SYMMETRIC_ATOMS;
  const int64_t ld = RYD_SC_NFIELD * nseg;

  struct Case {
    const char* name;
    ryd_sched_desc d;
    const double* table;
    int64_t ld_sched;
    int want;
    const char* msg;
  };
  std::vector<Case> cases;
  cases.push_back({"good descriptor, NULL handle", good, tab.data(), ld, RYD_ERR_INVALID, "handle is NULL"});
  cases.push_back({"NULL table", good, nullptr, ld, RYD_ERR_INVALID, "schedule table is NULL"});
  Case c = {"abi_version", good, tab.data(), ld, RYD_ERR_INVALID, "abi_version mismatch"};
  c.d.abi_version = RYD_ABI_VERSION + 1;
  cases.push_back(c);
  c = {"n_seg = 0", good, tab.data(), ld, RYD_ERR_INVALID, "n_seg must be"};
  c.d.n_seg = 0;
  cases.push_back(c);
  c = {"n_seg too large", good, tab.data(), ld, RYD_ERR_INVALID, "n_seg must be"};
  c.d.n_seg = RYD_SCHED_MAX_SEG + 1;
  cases.push_back(c);
  c = {"unknown flag", good, tab.data(), ld, RYD_ERR_INVALID, "unknown flag bits"};
  c.d.flags |= 64u;
  cases.push_back(c);
  c = {"dim 4", good, tab.data(), ld, RYD_ERR_UNSUPPORTED, "hilbert_space_dim 3 only"};
  c.d.dim = 4;
  cases.push_back(c);
  c = {"unequal atoms", good, tab.data(), ld, RYD_ERR_UNSUPPORTED, "identical atoms"};
  c.d.flags = 0;
  cases.push_back(c);
  cases.push_back({"ld_sched too small", good, tab.data(), ld - 1, RYD_ERR_INVALID, "ld_sched is smaller"});

  for (const Case& k : cases) {
    char what[96];
    std::snprintf(what, sizeof what, "ryd_run_schedule: %s", k.name);
    expect(what, ryd_run_schedule(nullptr, &k.d, p.data(), n, n, k.table, k.ld_sched, st.data(), 4 * n, sm.data(), n,
                                  status.data(), &stats), k.want, k.msg);
    std::snprintf(what, sizeof what, "ryd_run_schedule_kets: %s", k.name);
    expect(what, ryd_run_schedule_kets(nullptr, &k.d, p.data(), n, n, k.table, k.ld_sched, st.data(), 4 * n, sm.data(),
                                       n, jac.data(), ld, status.data(), &stats), k.want, k.msg);
    std::snprintf(what, sizeof what, "ryd_run_schedule_kets_ctl: %s", k.name);
    expect(what, ryd_run_schedule_kets_ctl(nullptr, &k.d, p.data(), n, n, k.table, k.ld_sched, st.data(), 4 * n,
                                           sm.data(), n, jac.data(), 4 * ld, status.data(), &stats), k.want, k.msg);
    std::snprintf(what, sizeof what, "ryd_run_schedule_coherences: %s", k.name);
    expect(what, ryd_run_schedule_coherences(nullptr, &k.d, p.data(), n, n, k.table, k.ld_sched, coh.data(), n,
                                             status.data(), &stats), k.want, k.msg);
  }
  // a NULL descriptor, the leading dimensions, and each family's own rules
  expect("ryd_run_schedule: NULL descriptor",
         ryd_run_schedule(nullptr, nullptr, p.data(), n, n, tab.data(), ld, st.data(), 4 * n, sm.data(), n,
                          status.data(), &stats), RYD_ERR_INVALID, "desc is NULL");
  expect("ryd_run_schedule: ld_state too small",
         ryd_run_schedule(nullptr, &good, p.data(), n, n, tab.data(), ld, st.data(), 4 * n - 1, sm.data(), n,
                          status.data(), &stats), RYD_ERR_INVALID, "leading dimension too small");
  expect("ryd_run_schedule: summary-only ignores ld_state",
         ryd_run_schedule(nullptr, &good, p.data(), n, n, tab.data(), ld, nullptr, 0, sm.data(), n, status.data(),
                          &stats), RYD_ERR_INVALID, "handle is NULL");
  expect("ryd_run_schedule_kets: ld_jac too small",
         ryd_run_schedule_kets(nullptr, &good, p.data(), n, n, tab.data(), ld, st.data(), 4 * n, sm.data(), n,
                               jac.data(), ld - 1, status.data(), &stats), RYD_ERR_INVALID, "ld_jac is smaller than 4");
  expect("ryd_run_schedule_kets: no Jacobian, ld_jac unread",
         ryd_run_schedule_kets(nullptr, &good, p.data(), n, n, tab.data(), ld, st.data(), 4 * n, sm.data(), n, nullptr,
                               0, status.data(), &stats), RYD_ERR_INVALID, "handle is NULL");
  expect("ryd_run_schedule_kets_ctl: NULL Jacobian",
         ryd_run_schedule_kets_ctl(nullptr, &good, p.data(), n, n, tab.data(), ld, st.data(), 4 * n, sm.data(), n,
                                   nullptr, 4 * ld, status.data(), &stats), RYD_ERR_INVALID, "control Jacobian is NULL");
  expect("ryd_run_schedule_kets_ctl: ld_jac too small",
         ryd_run_schedule_kets_ctl(nullptr, &good, p.data(), n, n, tab.data(), ld, st.data(), 4 * n, sm.data(), n,
                                   jac.data(), 4 * ld - 1, status.data(), &stats), RYD_ERR_INVALID,
         "ld_jac is smaller than 16");
  expect("ryd_run_schedule_coherences: ld_coh too small",
         ryd_run_schedule_coherences(nullptr, &good, p.data(), n, n, tab.data(), ld, coh.data(), n - 1, status.data(),
                                     &stats), RYD_ERR_INVALID, "leading dimension too small");
  // handle first
  expect("ryd_run_batch: NULL handle, NULL descriptor",
         ryd_run_batch(nullptr, nullptr, p.data(), n, n, st.data(), 4 * n, sm.data(), n, status.data(), &stats),
         RYD_ERR_INVALID, "handle is NULL");
  expect("ryd_run_coherences: NULL handle, NULL descriptor",
         ryd_run_coherences(nullptr, nullptr, p.data(), n, n, coh.data(), n, status.data(), &stats), RYD_ERR_INVALID,
         "handle is NULL");
  std::printf(bad ? "FAILED\n" : "all refusals as expected\n");
  return bad;
}
