// pack_sparse_check.cpp -- drives the host packer of slacken_amd/host/pack.hpp without a GPU, for a run under the host sanitizers:
// pack_bases_sparse against pack_bases over random text of all 256 byte values, at the sizes where the loops change (a word, a
// round of the SIMD route, a round of the exception scan), with buffers of exactly the documented sizes so that a byte too many
// is an error the sanitizer reports.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o pack_sparse_check tools/pack_sparse_check.cpp
//   ./pack_sparse_check
//
// Exit status 0: every check held.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../slacken_amd/host/pack.hpp"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "pack_sparse_check: %s failed (line %d, n = %llu)\n", #x, __LINE__, (unsigned long long)n); std::exit(1); } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

// mode 0: any byte; 1: nucleotides only (no exception); 2: an invalid base in every word; 3: nucleotides with a few N
static void one(uint64_t n, int mode) {
  std::vector<uint8_t> text(n);
  const char *nt = "ACGTacgtUu";
  for (uint64_t i = 0; i < n; i++) {
    text[i] = mode == 0 ? (uint8_t)rnd() : (uint8_t)nt[rnd() % 10];
    if (mode == 2 && i % 16 == rnd() % 16) text[i] = 'N';
    if (mode == 3 && rnd() % 97 == 0) text[i] = 'N';
  }
  if (mode == 2) for (uint64_t w = 0; w * 16 < n; w++) text[w * 16] = '-';
  const uint64_t words = (n + 15) / 16;
  std::vector<uint32_t> codes(words), dense_codes(words);
  std::vector<uint16_t> valid(words);
  slk::pack_bases(text.data(), n, dense_codes.data(), valid.data());
  // the count alone (no room at all), then exactly the room it asked for
  const uint64_t need = slk::pack_bases_sparse(text.data(), n, 0, codes.data(), nullptr, nullptr, 0, 0);
  CHECK(codes == dense_codes);
  std::vector<uint32_t> exc_word(need);
  std::vector<uint16_t> exc_bits(need);
  std::fill(codes.begin(), codes.end(), 0xDEADBEEFu);
  CHECK(slk::pack_bases_sparse(text.data(), n, 0, codes.data(), exc_word.data(), exc_bits.data(), 0, need) == need);
  CHECK(codes == dense_codes);
  std::vector<uint16_t> rebuilt(words);
  for (uint64_t w = 0; w < words; w++) rebuilt[w] = (uint16_t)((1u << (n - w * 16 < 16 ? n - w * 16 : 16)) - 1);
  for (uint64_t i = 0; i < need; i++) {
    CHECK(exc_word[i] < words && (i == 0 || exc_word[i] > exc_word[i - 1]));
    CHECK(exc_bits[i] != rebuilt[exc_word[i]]);   // (listed only where a base of the word is invalid)
    rebuilt[exc_word[i]] = exc_bits[i];
  }
  CHECK(rebuilt == valid);
  if (mode == 1) CHECK(need == 0);
  if (mode == 2) CHECK(need == words);
  // half the room: the first half is written, the count is still whole; a slice that starts at word 1000 names its words from there
  if (need >= 2) {
    std::vector<uint32_t> half_word(need / 2);
    std::vector<uint16_t> half_bits(need / 2);
    CHECK(slk::pack_bases_sparse(text.data(), n, 1000, codes.data(), half_word.data(), half_bits.data(), 0, need / 2) == need);
    for (uint64_t i = 0; i < need / 2; i++) CHECK(half_word[i] == exc_word[i] + 1000 && half_bits[i] == exc_bits[i]);
  }
}

int main() {
  const uint64_t sizes[] = {0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 16 * 2048 - 1, 16 * 2048, 16 * 2048 + 1, 100003};
  for (uint64_t n : sizes)
    for (int mode = 0; mode < 4; mode++) one(n, mode);
  std::printf("pack_sparse_check: ok\n");
  return 0;
}
