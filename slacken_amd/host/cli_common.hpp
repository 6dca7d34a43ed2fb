// cli_common.hpp -- what every part of the command-line host shares: the fatal error, the check of an slk_* call, the task timer,
// the wall clock, the cursor of the option loops, --devices and --shard-table, the size of the host's thread pools.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/slacken_amd.h"

namespace slk_host {

[[noreturn]] inline void die(const std::string &msg) {
  std::cerr << "slacken-amd: " << msg << std::endl;
  exit(2);
}
#define SLK_CALL(x) do { if ((x) != SLK_OK) die(std::string(#x) + ": " + slk_last_error()); } while (0)

inline double wall_seconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// wall-clock per sub-task, as Dynamic.Timer prints it (Dynamic.scala:46-54)
struct Timer {
  std::string task;
  double t0 = wall_seconds();
  explicit Timer(std::string t) : task(std::move(t)) {}
  ~Timer() { std::cerr << "Finish task: " << task << " [" << wall_seconds() - t0 << " s]" << std::endl; }
};

// The cursor of an option loop: `for (Args a(argc, argv); a.take();)` compares a with the options' names and asks for its value with a.next()
struct Args {
  int argc, i = 0;
  char **argv;
  std::string opt;   // the argument taken last
  Args(int argc_, char **argv_) : argc(argc_), argv(argv_) {}
  bool take() { return i < argc && (opt = argv[i++], true); }
  bool operator==(const char *name) const { return opt == name; }
  std::string next() { return i < argc ? argv[i++] : (die("missing value for " + opt), ""); }
  const char *peek() const { return i < argc ? argv[i] : nullptr; }   // (for the options that take a list of values)
};

inline std::vector<int> parse_device_list(const std::string &v) {   // --devices: `all` or e.g. 0,1,2,3
  std::vector<int> out;
  if (v == "all") {
    for (int d = 0; d < slk_device_count(); d++) out.push_back(d);
    if (out.empty()) die("--devices all: no GPU visible");
    return out;
  }
  size_t p0 = 0;
  while (p0 <= v.size()) {
    size_t p1 = v.find(',', p0);
    if (p1 == std::string::npos) p1 = v.size();
    if (p1 == p0 || !isdigit((unsigned char)v[p0])) die("--devices wants `all` or a comma-separated list of device numbers");
    out.push_back(std::stoi(v.substr(p0, p1 - p0)));
    p0 = p1 + 1;
  }
  return out;
}

// --devices of a command whose table must fit one GPU (`why` says which): `all` and lists are refused, --shard-table likewise
inline std::vector<int> parse_single_device(const std::string &v, const std::string &cmd, const std::string &why) {
  if (v == "all" || v.find(',') != std::string::npos) die(cmd + " takes one device: " + why);
  return parse_device_list(v);
}
[[noreturn]] inline void refuse_shard_table(const std::string &cmd, const std::string &why, const std::string &usage) {
  die("--shard-table is not supported by " + cmd + ": " + why + "\n" + usage);
}

inline std::ifstream open_input(const std::string &path) {
  std::ifstream f(path);
  if (!f) die("cannot open " + path);
  return f;
}
inline std::ofstream open_output(const std::string &path) {   // (with the directories above it)
  const std::filesystem::path p(path);
  if (p.has_parent_path()) std::filesystem::create_directories(p.parent_path());
  std::ofstream f(path);
  if (!f) die("cannot write " + path);
  return f;
}

inline size_t host_threads() {
  const char *e = getenv("SLK_HOST_THREADS");
  long v = e ? atol(e) : 0;
  if (v > 0) return (size_t)v;
  unsigned hc = std::thread::hardware_concurrency();
  return std::min<size_t>(32, std::max<unsigned>(2, hc) - 1);
}

}  // namespace slk_host
