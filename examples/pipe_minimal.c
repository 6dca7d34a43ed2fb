/* pipe_minimal.c -- two batches in flight from one thread (slk_pipe), the reads in the compact form: 2-bit codes, the validity as
 * a list of exception words, one length for all reads.   cc -Iinclude examples/pipe_minimal.c -Lslacken_amd/lib -lslacken_amd */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "slacken_amd.h"

#define CHECK(x) do { if ((x) != SLK_OK) { fprintf(stderr, "%s: %s\n", #x, slk_last_error()); return 1; } } while (0)
#define LEN 60   /* every read of this example has 60 bases */

int main(void) {
  const int32_t parents[5] = {0, 0, 1, 2, 2};   /* 1 = root, 2 = a genus, 3 and 4 = its species */
  slk_params p = {35, 31, 7, 1, SLK_DEFAULT_TOGGLE_MASK, 1, 0};
  slk_table_config cfg = {4096, 4, 0.0f};
  slk_index *ix = NULL;
  CHECK(slk_index_create(&p, &cfg, 0, &ix));
  CHECK(slk_index_set_taxonomy(ix, parents, 5));
  const char *g3 = "TAGGATCGATCGATCGGGATTTACGGCGATCTTAGGCTAGCTAGGCTTCGATATCGCGGCTATTAGCCGATTCGGA";
  const char *g4 = "CCATGGCTAGCTTAGGCGCGATATTCGGCTAGGATCCTAGGAGCTTCGAGGCTATATCGGCGGATTCGATCGTTAG";
  char seqs[256];
  snprintf(seqs, sizeof seqs, "%s%s", g3, g4);
  const uint64_t offsets[3] = {0, strlen(g3), strlen(g3) + strlen(g4)};
  const int32_t taxa[2] = {3, 4};
  CHECK(slk_index_add_sequences(ix, (const uint8_t *)seqs, offsets, taxa, 2));
  CHECK(slk_index_finalize(ix));

  /* two batches of two reads each; the second batch has an N in it.  The arrays are ordinary (pageable) memory, so they are free
   * again when slk_pipe_submit returns; memory of slk_host_alloc would have to stay unchanged until the collect. */
  char text[2][2 * LEN + 1];
  snprintf(text[0], sizeof text[0], "%.*s%.*s", LEN, g3, LEN, g4);
  snprintf(text[1], sizeof text[1], "%.*s%.*s", LEN, g4 + 10, LEN, g3 + 10);
  text[1][70] = 'N';
  slk_pipe *pipe = NULL;
  CHECK(slk_pipe_create(ix, 2, &pipe));
  const double thresholds[1] = {0.0};
  uint64_t ticket[2];
  for (int b = 0; b < 2; b++) {
    uint32_t codes[(2 * LEN + 15) / 16], exc_word[(2 * LEN + 15) / 16];
    uint16_t exc_bits[(2 * LEN + 15) / 16];
    uint64_t n_exc = 0;
    CHECK(slk_pack_bases_sparse((const uint8_t *)text[b], 2 * LEN, codes, exc_word, exc_bits, (2 * LEN + 15) / 16, &n_exc));
    slk_reads reads;
    memset(&reads, 0, sizeof reads);
    reads.codes = codes;
    reads.exc_word = n_exc ? exc_word : NULL;
    reads.exc_bits = n_exc ? exc_bits : NULL;
    reads.n_exc = n_exc;
    reads.uniform_len = LEN;
    CHECK(slk_pipe_submit(pipe, 2, &reads, NULL, 1, thresholds, 1, 2 /* hit lists */, &ticket[b]));   /* returns at once */
    printf("batch %d: %llu exception word(s), ticket %llu\n", b, (unsigned long long)n_exc, (unsigned long long)ticket[b]);
  }
  for (int b = 1; b >= 0; b--) {   /* any order */
    int32_t taxon[2], nd[2], tk[2];
    uint8_t cls[2];
    uint64_t hit_offs[3];
    slk_hit hits[256];
    CHECK(slk_pipe_collect(pipe, ticket[b], taxon, cls, nd, tk, hit_offs, hits, 256));
    for (int r = 0; r < 2; r++) {
      printf("batch %d read %d: taxon %d classified %d kmers %d hits", b, r, taxon[r], cls[r], tk[r]);
      for (uint64_t j = hit_offs[r]; j < hit_offs[r + 1]; j++) printf(" %d:%d", hits[j].taxon, hits[j].count);
      printf("\n");
    }
  }
  slk_pipe_destroy(pipe);
  slk_index_destroy(ix);
  return 0;
}
