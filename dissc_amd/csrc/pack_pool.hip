// Packing a model's layers on a few host threads (dissc_gen_create_ex collects one task per layer).  Host only: no kernel here.
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <exception>
#include <mutex>
#include <string>
#include <thread>

#include "common.h"

namespace dissc {

// default: min(8, the CPUs this process may really use / ranks on the node) -- hardware_concurrency() knows neither the cgroup
// CPU quota (the GPU boxes: 16 of 256 logical CPUs) nor that 8 ranks create handles at once
int pack_thread_count() {
  int nthr = 8;
  double cpus = (double)std::thread::hardware_concurrency();
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0};
    long long per = 0;
    if (fscanf(f, "%31s %lld", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) {
      const double quota = atof(q) / (double)per;
      if (quota >= 1.0 && (cpus <= 0 || quota < cpus)) cpus = quota;
    }
    fclose(f);
  }
  int ranks = 1;
  if (const char* e = getenv("LOCAL_WORLD_SIZE")) {
    const long v = strtol(e, nullptr, 10);
    if (v >= 1 && v <= 1024) ranks = (int)v;
  }
  if (cpus >= 1.0 && nthr > (int)(cpus / ranks)) nthr = (int)(cpus / ranks) > 1 ? (int)(cpus / ranks) : 1;
  if (const char* e = getenv("DISSC_PACK_THREADS")) {  // explicit override, validated
    char* end = nullptr;
    const long v = strtol(e, &end, 10);
    if (end != e && *end == 0 && v >= 1 && v <= 256) nthr = (int)v;
  }
  return nthr;
}

int run_pack_tasks(const std::vector<std::function<int()>>& tasks, int nthr, const Options& opt, int prec) {
  if (nthr > (int)tasks.size()) nthr = (int)tasks.size();  // (one thread: in place, on the caller's)
  int dev = 0;
  DISSC_HIP_CHECK(hipGetDevice(&dev));
  std::atomic<size_t> next{0};
  std::atomic<int> first_rc{DISSC_OK};
  std::mutex err_mu;
  std::string err_msg;
  auto worker = [&]() {
    if (hipSetDevice(dev) != hipSuccess) {
      first_rc = DISSC_EHIP;
      return;
    }
    OptScope scope(&opt);
    PrecScope prec_scope(prec);
    for (size_t i = next++; i < tasks.size() && first_rc == DISSC_OK; i = next++) {
      int r;
      try {
        r = tasks[i]();
      } catch (const std::exception& e) {  // (an exception leaving a std::thread would terminate the process)
        set_error("dissc_gen_create: packing a layer failed: %s", e.what());
        r = DISSC_ENOMEM;
      } catch (...) {
        set_error("dissc_gen_create: packing a layer failed (unknown exception)");
        r = DISSC_ENOMEM;
      }
      if (r != DISSC_OK) {
        std::lock_guard<std::mutex> lk(err_mu);
        if (first_rc == DISSC_OK) {
          first_rc = r;
          err_msg = dissc_last_error();  // the worker's thread-local message
        }
      }
    }
  };
  std::vector<std::thread> pool;
  try {
    for (int t = 0; t + 1 < nthr; ++t) pool.emplace_back(worker);
  } catch (const std::exception&) {  // no more threads to be had: whoever started shares the tasks with this thread
  }
  worker();  // the creating thread packs too (and alone, if no thread could be started)
  for (auto& t : pool) t.join();
  if (first_rc != DISSC_OK) set_error("%s", err_msg.empty() ? "dissc_gen_create: a packing thread failed" : err_msg.c_str());
  return first_rc;
}

}  // namespace dissc
