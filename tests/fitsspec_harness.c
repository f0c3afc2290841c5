/* Stand-alone driver of csrc/fitsspec.c for the sanitiser run of tests/test_fits.py: every path of
 * argv is read (good files, truncated ones, wrong headers, a missing one), singly and as one list. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int gpdla_fitsspec_sizes(const char **, int64_t, int64_t *, int64_t *, int64_t *, char *, int, int);
int gpdla_fitsspec_read(const char **, int64_t, const int64_t *, const int64_t *, const int64_t *, float *, float *, float *,
                        int32_t *, char *, int, int);

static int run(const char **paths, int64_t n, int threads, double *sum) {
  int64_t *counts = calloc(n + 1, 8), *off = calloc(n + 1, 8), *rb = calloc(n + 1, 8), *offsets = calloc(n + 2, 8);
  char err[256] = "";
  int rc = gpdla_fitsspec_sizes(paths, n, counts, off, rb, err, sizeof err, threads);
  if (!rc) {
    for (int64_t i = 0; i < n; i++) offsets[i + 1] = offsets[i] + counts[i];
    const int64_t total = offsets[n];
    float *f = malloc(total * 4 + 4), *l = malloc(total * 4 + 4), *v = malloc(total * 4 + 4);
    int32_t *m = malloc(total * 4 + 4);
    rc = gpdla_fitsspec_read(paths, n, offsets, off, rb, f, l, v, m, err, sizeof err, threads);
    if (!rc)
      for (int64_t j = 0; j < total; j++) *sum += l[j] + (m[j] & 1);
    free(f); free(l); free(v); free(m);
  }
  if (rc) printf("refused (%d): %s\n", rc, err);
  free(counts); free(off); free(rb); free(offsets);
  return rc;
}

int main(int argc, char **argv) {
  const char **paths = (const char **)(argv + 1);
  const int64_t n = argc - 1;
  long ok = 0, bad = 0;
  double sum = 0.0;
  for (int64_t i = 0; i < n; i++) {
    if (run(paths + i, 1, 1, &sum)) bad++;
    else ok++;
  }
  run(paths, n, 4, &sum);                       /* the list as a whole: stops at its first bad file */
  const char **with_null = calloc(n + 1, sizeof *with_null);
  for (int64_t i = 0; i < n; i++) with_null[i + 1] = paths[i];
  run(with_null, n ? 2 : 1, 2, &sum);           /* a NULL path: no pixel */
  free(with_null);
  /* a tiny error buffer must be respected */
  char tiny[8];
  int64_t a, b, c;
  const char *missing = "/nonexistent/spec-0-0-0000.fits";
  gpdla_fitsspec_sizes(&missing, 1, &a, &b, &c, tiny, sizeof tiny, 1);
  printf("ok %ld, refused %ld of %ld (checksum %.6g)\n", ok, bad, (long)n, sum);
  return 0;
}
