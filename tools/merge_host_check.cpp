// merge_host_check.cpp -- drives the host-only parts of slacken_amd/host/merge.hpp without a GPU, for a run under the host
// sanitizers: the translation of a source's taxa into a destination taxonomy (taxon_remap) on hand-written trees, and what `merge`
// compares of the sources' .properties files.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o merge_host_check tools/merge_host_check.cpp
//       -Lslacken_amd/lib -lslacken_amd -lz -ldl -lpthread -Wl,-rpath,$PWD/slacken_amd/lib          (one command line)
//   ./merge_host_check SCRATCH_DIR
//
// SCRATCH_DIR: an existing directory; two .properties stubs are written there.  Exit status 0: every check held.
#include <cstdio>
#include <cstdlib>

#include "../slacken_amd/host/merge.hpp"

using namespace slk_host;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "merge_host_check: %s failed (line %d)\n", #x, __LINE__); std::exit(1); } } while (0)

using Nodes = std::vector<std::tuple<Taxon, Taxon, std::string>>;

static Taxonomy tree(const Nodes &nodes, const std::vector<std::pair<Taxon, Taxon>> &merged = {}) {
  return Taxonomy::fromNodesAndNames(nodes, {}, merged);
}

static void write_stub(const std::string &loc, int k, int m, int spaces, const char *extra) {
  std::ofstream f = open_output(loc + ".properties");
  f << "k=" << k << "\nm=" << m << "\nversion=1\nsplitter=randomXOR\nminimizerSpaces=" << spaces << "\n" << extra;
}

int main(int argc, char **argv) {
  if (argc != 2) die("usage: merge_host_check SCRATCH_DIR");
  // src defines 1 2 3 4 5 7
  const Nodes src_nodes = {{1, 1, "no rank"}, {2, 1, "genus"}, {3, 1, "genus"}, {4, 2, "species"}, {5, 2, "species"}, {7, 3, "species"}};
  const Taxonomy src = tree(src_nodes);
  using V = std::vector<int32_t>;
  TaxonRemap r = taxon_remap(src, tree(src_nodes));
  CHECK(r.identity && r.map == (V{0, 1, 2, 3, 4, 5, 0, 7}));
  Nodes larger = src_nodes;
  larger.push_back({6, 3, "species"});
  larger.push_back({8, 1, "genus"});
  r = taxon_remap(src, tree(larger));
  CHECK(r.identity && r.map == (V{0, 1, 2, 3, 4, 5, 0, 7}));
  const Nodes without5 = {{1, 1, "no rank"}, {2, 1, "genus"}, {3, 1, "genus"}, {4, 2, "species"}, {7, 3, "species"}};
  r = taxon_remap(src, tree(without5, {{5, 4}}));          // merged.dmp: 5 went into 4
  CHECK(!r.identity && r.map == (V{0, 1, 2, 3, 4, 4, 0, 7}));
  r = taxon_remap(src, tree(without5));                    // 5 is gone and nothing says where
  CHECK(!r.identity && r.map == (V{0, 1, 2, 3, 4, 0, 0, 7}));
  r = taxon_remap(src, tree(without5, {{5, 6}}));          // ... or it went into a node the destination does not define
  CHECK(!r.identity && r.map == (V{0, 1, 2, 3, 4, 0, 0, 7}));
  const Nodes short_nodes = {{1, 1, "no rank"}, {2, 1, "genus"}, {3, 1, "genus"}, {4, 2, "species"}, {5, 2, "species"}};
  r = taxon_remap(src, tree(short_nodes));                 // 7 lies beyond the destination's arrays
  CHECK(!r.identity && r.map == (V{0, 1, 2, 3, 4, 5, 0, 0}));
  r = taxon_remap(tree({{1, 1, "no rank"}}), tree(short_nodes));   // the smallest source there is
  CHECK(r.identity && r.map == (V{0, 1}));

  // the fields merge compares
  const IndexParams a{35, 31, 7, SLK_DEFAULT_TOGGLE_MASK, true};
  auto differs = [&](IndexParams b) { const char *f = differing_splitter_field(a, b); return std::string(f ? f : ""); };
  CHECK(differs(a) == "");
  CHECK(differs({33, 31, 7, a.xorMask, true}) == "k" && differs({35, 29, 7, a.xorMask, true}) == "m");
  CHECK(differs({35, 31, 9, a.xorMask, true}) == "minimizerSpaces" && differs({35, 31, 7, 5, true}) == "XORmask");
  CHECK(differs({35, 31, 7, a.xorMask, false}) == "canonical");
  const std::string dir = argv[1];
  write_stub(dir + "/one", 35, 31, 7, "");
  write_stub(dir + "/two", 35, 31, 7, "canonical=true\n");
  const IndexParams got = check_merge_sources(dir + "/out", {dir + "/one", dir + "/two", dir + "/one"});
  CHECK(got.k == 35 && got.m == 31 && got.spaces == 7 && got.canonical && got.xorMask == SLK_DEFAULT_TOGGLE_MASK);
  std::printf("merge_host_check: all checks held\n");
  return 0;
}
