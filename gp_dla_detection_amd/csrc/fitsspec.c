/* fitsspec.c -- columns 1-4 of HDU 1 (flux E, loglam E, ivar E, and_mask J) of many SDSS spec files,
 * read in threads into one CSR set.  Host code only; built by
 * io.build_fitsspec() with gcc -O2 -fopenmp; gp_dla_detection_amd/fits.py reads the same arrays without it.
 *
 * Two passes: gpdla_fitsspec_sizes parses the two headers of every file (row count, where the table
 * starts, the row length) and checks the first four columns by TFORM and, case-insensitively, by
 * TTYPE; gpdla_fitsspec_read then copies the big-endian columns into flat float32 / int32 arrays at
 * the offsets the caller derived from the counts.  Both return 0, or -- with a message that names the
 * file and the card in err -- the 1-based index of the FIRST file that failed, whichever thread met
 * it.  A NULL path stands for a quasar that is not read: no pixel.
 */
#define _GNU_SOURCE
#include <ctype.h>
#include <fcntl.h>
#include <sched.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#define BLOCK 2880
#define CARD 80
#define MAX_HEADER_BLOCKS 64

static void say(char *err, int errlen, const char *fmt, ...) {
  if (!err || errlen <= 0) return;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err, (size_t)errlen, fmt, ap);
  va_end(ap);
}

static int thread_count(int asked) {
  int n = asked;
  if (n <= 0) {
    cpu_set_t set;
    n = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : 1;
  }
  if (n > 16) n = 16;
  return n < 1 ? 1 : n;
}

/* keyword of a card, blanks trimmed, into key[9] */
static void card_key(const char *card, char *key) {
  int n = 8;
  while (n > 0 && card[n - 1] == ' ') --n;
  memcpy(key, card, (size_t)n);
  key[n] = 0;
}

static int has_value(const char *card) { return card[8] == '=' && card[9] == ' '; }

/* integer value of a card; 0 on success */
static int card_int(const char *card, int64_t *out) {
  char buf[CARD - 10 + 1];
  memcpy(buf, card + 10, CARD - 10);
  buf[CARD - 10] = 0;
  char *slash = strchr(buf, '/');
  if (slash) *slash = 0;
  char *end;
  const long long v = strtoll(buf, &end, 10);
  if (end == buf) return -1;
  while (*end == ' ') ++end;
  if (*end) return -1;
  *out = v;
  return 0;
}

/* floating value of a card (TSCAL / TZERO); 0 on success */
static int card_double(const char *card, double *out) {
  char buf[CARD - 10 + 1];
  memcpy(buf, card + 10, CARD - 10);
  buf[CARD - 10] = 0;
  char *slash = strchr(buf, '/');
  if (slash) *slash = 0;
  for (char *p = buf; *p; ++p)
    if (*p == 'D' || *p == 'd') *p = 'E';
  char *end;
  const double v = strtod(buf, &end);
  if (end == buf) return -1;
  while (*end == ' ') ++end;
  if (*end) return -1;
  *out = v;
  return 0;
}

/* string value of a card ('' is one quote, trailing blanks dropped) into out[CARD]; 0 on success */
static int card_string(const char *card, char *out) {
  int i = 10, n = 0;
  while (i < CARD && card[i] == ' ') ++i;
  if (i >= CARD || card[i] != '\'') return -1;
  for (++i; i < CARD; ++i) {
    if (card[i] == '\'') {
      if (i + 1 < CARD && card[i + 1] == '\'') {
        out[n++] = '\'';
        ++i;
        continue;
      }
      while (n > 0 && out[n - 1] == ' ') --n;
      out[n] = 0;
      return 0;
    }
    out[n++] = card[i];
  }
  return -1;
}

typedef struct {
  int64_t bitpix, naxis, axes_product, pcount, gcount, naxis1, naxis2, tfields;
  int has_xtension, is_bintable, has_simple;
  char tform[4][CARD], ttype[4][CARD];
  int has_tform[4], has_ttype[4];
  double tscal[4], tzero[4];
} header_t;

/* Parses the header that starts at *pos; leaves *pos at the first byte after its last block.
 * 0, or -1 with a message. */
static int parse_header(int fd, const char *path, int64_t size, int64_t *pos, int hdu, header_t *h, char *err, int errlen) {
  char block[BLOCK], key[9];
  memset(h, 0, sizeof(*h));
  h->axes_product = 1;
  h->gcount = 1;
  for (int c = 0; c < 4; ++c) {
    h->tscal[c] = 1.0;
    h->tzero[c] = 0.0;
  }
  for (int b = 0; b < MAX_HEADER_BLOCKS; ++b) {
    if (*pos + BLOCK > size || pread(fd, block, BLOCK, (off_t)*pos) != BLOCK) {
      say(err, errlen, "%s: truncated in the header of HDU %d", path, hdu);
      return -1;
    }
    *pos += BLOCK;
    for (int c = 0; c < BLOCK; c += CARD) {
      const char *card = block + c;
      card_key(card, key);
      if (!strcmp(key, "END")) return 0;
      if (!has_value(card) || !strcmp(key, "COMMENT") || !strcmp(key, "HISTORY") || !strcmp(key, "CONTINUE") || !key[0])
        continue;
      int64_t v;
      int bad = 0;
      if (!strcmp(key, "SIMPLE")) h->has_simple = 1;
      else if (!strcmp(key, "XTENSION")) {
        char s[CARD];
        h->has_xtension = 1;
        h->is_bintable = card_string(card, s) == 0 && !strcmp(s, "BINTABLE");
      } else if (!strcmp(key, "BITPIX")) bad = card_int(card, &h->bitpix);
      else if (!strcmp(key, "NAXIS")) bad = card_int(card, &h->naxis);
      else if (!strcmp(key, "PCOUNT")) bad = card_int(card, &h->pcount);
      else if (!strcmp(key, "GCOUNT")) bad = card_int(card, &h->gcount);
      else if (!strcmp(key, "TFIELDS")) bad = card_int(card, &h->tfields);
      else if (!strncmp(key, "NAXIS", 5) && isdigit((unsigned char)key[5])) {
        bad = card_int(card, &v);
        if (!bad) {
          if (v < 0 || (v > 0 && h->axes_product > INT64_MAX / 16 / v)) bad = 1;
          else h->axes_product *= v;
          if (!strcmp(key, "NAXIS1")) h->naxis1 = v;
          if (!strcmp(key, "NAXIS2")) h->naxis2 = v;
        }
      } else if ((!strncmp(key, "TFORM", 5) || !strncmp(key, "TTYPE", 5) || !strncmp(key, "TSCAL", 5) || !strncmp(key, "TZERO", 5)) &&
                 key[5] >= '1' && key[5] <= '4' && !key[6]) {
        const int col = key[5] - '1';
        if (key[1] == 'F') bad = card_string(card, h->tform[col]), h->has_tform[col] = !bad;
        else if (key[1] == 'T') bad = card_string(card, h->ttype[col]), h->has_ttype[col] = !bad;
        else if (key[1] == 'S') bad = card_double(card, &h->tscal[col]);
        else bad = card_double(card, &h->tzero[col]);
      }
      if (bad) {
        say(err, errlen, "%s: HDU %d: cannot parse the card %s", path, hdu, key);
        return -1;
      }
    }
  }
  say(err, errlen, "%s: the header of HDU %d has no END card in %d blocks", path, hdu, MAX_HEADER_BLOCKS);
  return -1;
}

static int same_nocase(const char *a, const char *b) {
  for (; *a && *b; ++a, ++b)
    if (tolower((unsigned char)*a) != tolower((unsigned char)*b)) return 0;
  return !*a && !*b;
}

/* the layout of HDU 1 of one file; 0, or -1 with a message */
static int spec_layout(const char *path, int64_t *rows, int64_t *data_off, int64_t *row_bytes, char *err, int errlen) {
  static const char *names[4] = {"flux", "loglam", "ivar", "and_mask"};
  static const char letters[4] = {'E', 'E', 'E', 'J'};
  const int fd = open(path, O_RDONLY);
  if (fd < 0) {
    say(err, errlen, "%s cannot be opened", path);
    return -1;
  }
  struct stat st;
  int rc = -1;
  header_t h;
  int64_t pos = 0;
  if (fstat(fd, &st) != 0) {
    say(err, errlen, "%s cannot be opened", path);
    goto done;
  }
  if (parse_header(fd, path, st.st_size, &pos, 0, &h, err, errlen)) goto done;
  if (!h.has_simple) {
    say(err, errlen, "%s: HDU 0 does not start with SIMPLE", path);
    goto done;
  }
  {
    const int64_t ab = h.bitpix < 0 ? -h.bitpix : h.bitpix;
    const int64_t bytes = h.naxis == 0 ? 0 : ab / 8 * h.gcount * (h.pcount + h.axes_product);
    if (bytes < 0 || bytes > st.st_size) {
      say(err, errlen, "%s: truncated in the data of HDU 0", path);
      goto done;
    }
    pos += (bytes + BLOCK - 1) / BLOCK * BLOCK;
  }
  if (pos >= st.st_size) {
    say(err, errlen, "%s: no HDU 1", path);
    goto done;
  }
  if (parse_header(fd, path, st.st_size, &pos, 1, &h, err, errlen)) goto done;
  if (!h.has_xtension || !h.is_bintable) {
    say(err, errlen, "%s: HDU 1 is not a binary table (XTENSION)", path);
    goto done;
  }
  if (h.tfields < 4) {
    say(err, errlen, "%s: TFIELDS = %lld: HDU 1 needs the four columns flux, loglam, ivar, and_mask", path, (long long)h.tfields);
    goto done;
  }
  for (int c = 0; c < 4; ++c) {
    const char *f = h.tform[c];
    if (!h.has_tform[c] || !((f[0] == letters[c] && !f[1]) || (f[0] == '1' && f[1] == letters[c] && !f[2]))) {
      say(err, errlen, "%s: TFORM%d = '%s', expected '%c'", path, c + 1, h.has_tform[c] ? f : "", letters[c]);
      goto done;
    }
    if (!h.has_ttype[c] || !same_nocase(h.ttype[c], names[c])) {
      say(err, errlen, "%s: TTYPE%d = '%s', expected '%s'", path, c + 1, h.has_ttype[c] ? h.ttype[c] : "", names[c]);
      goto done;
    }
    if (h.tscal[c] != 1.0 || h.tzero[c] != 0.0) {
      say(err, errlen, "%s: TSCAL%d / TZERO%d = %g / %g: scaled columns are not read", path, c + 1, c + 1, h.tscal[c], h.tzero[c]);
      goto done;
    }
  }
  if (h.naxis1 < 16 || h.naxis2 < 0 || h.naxis2 > INT32_MAX) {
    say(err, errlen, "%s: HDU 1: NAXIS1 = %lld, NAXIS2 = %lld", path, (long long)h.naxis1, (long long)h.naxis2);
    goto done;
  }
  if (h.naxis1 > (st.st_size - pos) / (h.naxis2 > 0 ? h.naxis2 : 1)) {
    say(err, errlen, "%s: truncated in the data of HDU 1", path);
    goto done;
  }
  *rows = h.naxis2;
  *data_off = pos;
  *row_bytes = h.naxis1;
  rc = 0;
done:
  close(fd);
  return rc;
}

static uint32_t be32(const unsigned char *p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

/* the table of one file into the flat arrays at `at`; 0, or -1 with a message */
static int spec_read(const char *path, int64_t rows, int64_t data_off, int64_t row_bytes, int64_t at, float *flux,
                     float *loglam, float *ivar, int32_t *and_mask, char *err, int errlen) {
  if (rows == 0) return 0;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) {
    say(err, errlen, "%s cannot be opened", path);
    return -1;
  }
  const size_t bytes = (size_t)rows * (size_t)row_bytes;
  unsigned char *buf = (unsigned char *)malloc(bytes);
  int rc = -1;
  if (!buf) {
    say(err, errlen, "%s: out of memory for %zu bytes", path, bytes);
    goto done;
  }
  for (size_t got = 0; got < bytes;) {
    const ssize_t r = pread(fd, buf + got, bytes - got, (off_t)(data_off + (int64_t)got));
    if (r <= 0) {
      say(err, errlen, "%s: truncated in the data of HDU 1", path);
      goto done;
    }
    got += (size_t)r;
  }
  uint32_t *dst[4] = {(uint32_t *)(flux + at), (uint32_t *)(loglam + at), (uint32_t *)(ivar + at), (uint32_t *)(and_mask + at)};
  for (int64_t r = 0; r < rows; ++r) {
    const unsigned char *row = buf + (size_t)r * (size_t)row_bytes;
    for (int c = 0; c < 4; ++c) dst[c][r] = be32(row + 4 * c);
  }
  rc = 0;
done:
  free(buf);
  close(fd);
  return rc;
}

int gpdla_fitsspec_sizes(const char **paths, int64_t n, int64_t *counts, int64_t *data_off, int64_t *row_bytes,
                         char *err, int errlen, int threads) {
  int64_t first_bad = n;
  const int nt = thread_count(threads);
#pragma omp parallel for schedule(dynamic, 16) num_threads(nt) reduction(min : first_bad)
  for (int64_t i = 0; i < n; ++i) {
    counts[i] = data_off[i] = row_bytes[i] = 0;
    if (!paths[i]) continue;
    if (spec_layout(paths[i], &counts[i], &data_off[i], &row_bytes[i], NULL, 0) && i < first_bad) first_bad = i;
  }
  if (first_bad == n) return 0;
  int64_t a, b, c;   /* the message of the first failure, whichever thread met it */
  if (!spec_layout(paths[first_bad], &a, &b, &c, err, errlen)) say(err, errlen, "%s changed while it was read", paths[first_bad]);
  return (int)(first_bad < INT32_MAX - 1 ? first_bad + 1 : INT32_MAX);
}

int gpdla_fitsspec_read(const char **paths, int64_t n, const int64_t *offsets, const int64_t *data_off,
                        const int64_t *row_bytes, float *flux, float *loglam, float *ivar, int32_t *and_mask, char *err,
                        int errlen, int threads) {
  int64_t first_bad = n;
  const int nt = thread_count(threads);
#pragma omp parallel for schedule(dynamic, 16) num_threads(nt) reduction(min : first_bad)
  for (int64_t i = 0; i < n; ++i) {
    if (!paths[i]) continue;
    if (spec_read(paths[i], offsets[i + 1] - offsets[i], data_off[i], row_bytes[i], offsets[i], flux, loglam, ivar,
                  and_mask, NULL, 0) && i < first_bad)
      first_bad = i;
  }
  if (first_bad == n) return 0;
  /* read it once more into scratch for the message: the output arrays keep whatever was written */
  const int64_t rows = offsets[first_bad + 1] - offsets[first_bad];
  float *tmp = (float *)malloc((size_t)(rows > 0 ? rows : 1) * 16);
  if (!tmp || !spec_read(paths[first_bad], rows, data_off[first_bad], row_bytes[first_bad], 0, tmp, tmp + rows, tmp + 2 * rows,
                         (int32_t *)(tmp + 3 * rows), err, errlen))
    say(err, errlen, "%s changed while it was read", paths[first_bad]);
  free(tmp);
  return (int)(first_bad < INT32_MAX - 1 ? first_bad + 1 : INT32_MAX);
}
