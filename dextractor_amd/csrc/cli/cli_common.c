#define _GNU_SOURCE
/*
 * cli_common.c -- command-line surface of the reference's six codec tools, on top of libdexgpu.
 *
 * Same flags, usage text, file naming (<dir>/<root><.ext>), -i pipe mode, -v messages, source
 * removal unless -k, error messages and exit codes as dexta.c / undexta.c / dexar.c / undexar.c /
 * dexqv.c / undexqv.c (argument macros DB.h:79-123, path helpers DB.c:112-181).  A file goes to the
 * GPU through one of libdexgpu's file drivers, by the first of these routes whose precondition holds:
 *   1. dexqv of a large file on one context: read from the descriptor, written at the output's offsets
 *   2. dexta / dexar with -i, or of a very large file on one context: streamed, a chunk of records at a time
 *   3. undexta / undexar with -i: streamed likewise
 *      (from here on the input is read whole)
 *   4. undexqv on one context: by a plan of its records, into the output file or, for a pipe, through memory
 *   5. dexqv on one context, undexta, undexar into a file of ours: chunk by chunk at the output's offsets
 *   6. everything else, a file sharded over several contexts included: converted and written whole
 * There is no CPU codec here: without a HIP device the tools fail loudly.
 */
#include <pthread.h>
#include <sys/stat.h>
#include <sys/mman.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <time.h>
#include <unistd.h>

#include "cli_common.h"
#include "dexgpu.h"
#include "../dx_env.h"

typedef struct
  { const char *name, *flags, *src_ext, *dst_ext, *what, *usage;
    int         pipe_ok;
    const char *help[4];
  } tool_t;

static const tool_t TOOLS[6] =
  { { "dexta",   "vki",  ".fasta", ".dexta", "Fasta", "[-vk] ( -i | <path:fasta> ... )", 1,
      { "      -i: source is on standard input.\n",
        "      -k: do *not* remove the .fasta file on completion.\n",
        "      -w: line width for sequence lines.\n", NULL } },
    { "undexta", "vkiU", ".dexta", ".fasta", "dexta", "[-vkU] [-w<int(80)>] ( -i | <path:dexta> ... )", 1,
      { "      -i: source is on standard input.\n",
        "      -k: do *not* remove the .dexta file on completion.\n",
        "      -U: use uppercase letters (default is lower case).\n",
        "      -w: line width for sequence lines.\n" } },
    { "dexar",   "vki",  ".arrow", ".dexar", "Arrow", "[-vk] ( -i | <path:arrow> ... )", 1,
      { "      -i: source is on standard input.\n",
        "      -k: do *not* remove the .arrow file on completion.\n", NULL, NULL } },
    { "undexar", "vki",  ".dexar", ".arrow", "dexar", "[-vk] [-w<int(80)>] ( -i | <path:dexar> ... )", 1,
      { "      -i: source is on standard input.\n",
        "      -k: do *not* remove the .dexar file on completion.\n",
        "      -w: line width for arrow lines.\n", NULL } },
    { "dexqv",   "vkl",  ".quiva", ".dexqv", "quiva", "[-vkl] <path:quiva> ...", 0,
      { "      -k: do *not* remove the .quiva file on completion.\n",
        "      -l: use lossy compression (not recommended).\n", NULL, NULL } },
    { "undexqv", "vkU",  ".dexqv", ".quiva", "dexqv", "[-vkU] <path:dexqv> ...", 0,
      { "      -k: do *not* remove the .dexqv file on completion.\n",
        "      -U: use uppercase letters (default is lower case).\n", NULL, NULL } } };

static const char *Prog;
static int         Digest = 0;   /* DEXGPU_DIGEST: 1: a line on stdout for every file done; 2 ("only"): the line, and no output file */
static int         Census = 0;   /* DEXGPU_CENSUS: the same for the census line (it follows the digest's) */
#define LINES_ONLY (Digest == 2 || Census == 2)

/* ---- whole-file I/O ---------------------------------------------------------------------- */

/* The whole input as one buffer.  A regular file is mapped (no copy through a read buffer: the
   upload to the GPU reads the page cache directly); a pipe is read to its end.  *mapped tells
   unslurp which. */
static uint8_t *slurp(FILE *f, size_t *n, int *mapped)
{ size_t cap = 1 << 20, len = 0, k;
  uint8_t *buf;
  struct stat st;
  *mapped = 0;
  if (fstat(fileno(f), &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0)
    { void *m = mmap(NULL, (size_t) st.st_size, PROT_READ, MAP_PRIVATE, fileno(f), 0);
      if (m != MAP_FAILED)
        { /* pages brought in 16 MiB at a time rather than with MAP_POPULATE: one long populate holds the address
             space's lock against the GPU runtime that is starting up on the other thread (its own mmaps then
             wait for the whole read: 100 -> 185 ms of context creation beside a 1 GB file) */
#ifdef MADV_POPULATE_READ
          size_t at;
          for (at = 0; at < (size_t) st.st_size; at += (size_t) 16 << 20)
            { size_t piece = (size_t) st.st_size - at < ((size_t) 16 << 20) ? (size_t) st.st_size - at : (size_t) 16 << 20;
              if (madvise((uint8_t *) m + at, piece, MADV_POPULATE_READ) != 0)
                break;                                   /* (older kernel: the pages fault in when they are read) */
            }
#endif
          *mapped = 1;
          *n = (size_t) st.st_size;
          return (uint8_t *) m;
        }
      cap = (size_t) st.st_size + 1;
    }
  buf = malloc(cap);
  if (buf == NULL) return NULL;
  while ((k = fread(buf + len, 1, cap - len, f)) > 0)
    { len += k;
      if (len == cap)
        { uint8_t *nb = realloc(buf, cap *= 2);
          if (nb == NULL) { free(buf); return NULL; }
          buf = nb;
        }
    }
  *n = len;
  return buf;
}

/* The whole output image to a regular file: large images through a shared mapping of the file that several
   threads fill, a slice each (write() calls on one file queue up behind its inode lock, page faults on a
   mapping do not).  The file's pages are allocated first, in one posix_fallocate call: threads that fault
   fresh pages into one file contend for its page-cache lock (1 GiB to tmpfs, 8 threads: 2.6 s; allocated
   first: 0.09 s + 0.12 s of copying), and a full file system is an error return instead of a SIGBUS.
   Pipes, small outputs and anything that cannot be mapped go by fwrite.  0 on success.                    */
typedef struct { uint8_t *dst; const uint8_t *src; size_t n; } wjob;

static void *copy_slice(void *arg)
{ wjob *j = arg;
  memcpy(j->dst, j->src, j->n);
  return NULL;
}

/* May the output be laid out directly in the file behind f (posix_fallocate / ftruncate / pwrite at absolute
   offsets / a mapping)?  Only when the file is ours to lay out: a regular file that is empty, positioned at its
   start and not opened for appending.  `tool -i <in >>all` (O_APPEND: pwrite appends whatever the offset, ftruncate
   would cut what is there) and `1<>file` (existing bytes behind offset 0) go through fwrite like a pipe.           */
static int file_is_ours(FILE *f)
{ struct stat st;
  int fd = fileno(f), fl;
  if (fflush(f) != 0 || fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size != 0) return 0;
  if ((fl = fcntl(fd, F_GETFL)) < 0 || (fl & O_APPEND)) return 0;
  return lseek(fd, 0, SEEK_CUR) == 0;
}

static int write_image(FILE *f, const uint8_t *buf, size_t n)
{ long cores = sysconf(_SC_NPROCESSORS_ONLN);
  int  T = cores > 16 ? 16 : (int) cores, k, made = 0;
  uint8_t *map;
  if (n < ((size_t) 32 << 20) || T < 2 || !file_is_ours(f) || posix_fallocate(fileno(f), 0, (off_t) n) != 0 ||
      ftruncate(fileno(f), (off_t) n) != 0)
    return (n > 0 && fwrite(buf, 1, n, f) != n) ? -1 : 0;
  map = mmap(NULL, n, PROT_READ | PROT_WRITE, MAP_SHARED, fileno(f), 0);
  if (map == MAP_FAILED)
    return (fwrite(buf, 1, n, f) != n) ? -1 : 0;
  { wjob      job[16];
    pthread_t th[16];
    size_t    slice = (n / (size_t) T + 4095) & ~(size_t) 4095;
    for (k = 0; k < T; k++)
      { size_t lo = (size_t) k * slice, hi = lo + slice < n ? lo + slice : n;
        if (lo >= n) break;
        job[k].dst = map + lo; job[k].src = buf + lo; job[k].n = hi - lo;
        if (k > 0 && pthread_create(&th[k], NULL, copy_slice, &job[k]) != 0)
          { copy_slice(&job[k]);                          /* no thread to be had: this one does the slice */
            th[k] = pthread_self();
          }
        made = k + 1;
      }
    copy_slice(&job[0]);
    for (k = 1; k < made; k++)
      if (!pthread_equal(th[k], pthread_self())) pthread_join(th[k], NULL);
  }
  if (munmap(map, n) != 0) return -1;
  return lseek(fileno(f), (off_t) n, SEEK_SET) < 0 ? -1 : 0;
}

static void unslurp(uint8_t *buf, size_t n, int mapped)
{ if (mapped) munmap(buf, n);
  else        free(buf);
}

/* directory part / root name, as PathTo and Root do (DB.c:112-160) */
static char *path_to(const char *name)
{ const char *s = strrchr(name, '/');
  char *p;
  if (s == NULL) return strdup(".");
  p = malloc((size_t) (s - name) + 1);
  memcpy(p, name, (size_t) (s - name));
  p[s - name] = '\0';
  return p;
}

static char *root_of(const char *name, const char *suffix)
{ const char *f = strrchr(name, '/');
  size_t fl, sl = strlen(suffix);
  char  *r;
  f  = f ? f + 1 : name;
  fl = strlen(f);
  r  = strdup(f);
  if (fl > sl && strcasecmp(f + (fl - sl), suffix) == 0)
    r[fl - sl] = '\0';
  return r;
}

static char *catenate(const char *dir, const char *root, const char *ext)
{ char *p = malloc(strlen(dir) + strlen(root) + strlen(ext) + 2);
  sprintf(p, "%s/%s%s", dir, root, ext);
  return p;
}

/* ---- error reporting in the reference's words ------------------------------------------------ */

static void report_text_error(int tool, uint64_t line, int code)
{ const tool_t *t = &TOOLS[tool];
  if (tool == TOOL_DEXQV)
    switch (code)
      { case DX_IDX_NO_NEWLINE: fprintf(stderr, "Line %llu: Last line does not end with a newline !\n", (unsigned long long) line); break;   /* QV.c:779 */
        case DX_IDX_NO_HEADER:  fprintf(stderr, "Line %llu: Header in quiva file is missing\n", (unsigned long long) line); break;          /* QV.c:955 */
        case DX_IDX_INCOMPLETE: fprintf(stderr, "Line %llu: incomplete last entry of .quiv file\n", (unsigned long long) line); break;      /* QV.c:789 */
        case DX_IDX_RAGGED:     fprintf(stderr, "Line %llu: Lines for an entry are not the same length\n", (unsigned long long) line); break; /* QV.c:793 */
        default:                fprintf(stderr, "%s: Line %llu: Header line incorrectly formatted ?\n", Prog, (unsigned long long) line); break; /* QV.c:960 */
      }
  else
    switch (code)
      { case DX_IDX_TOO_LONG:
        case DX_IDX_NO_NEWLINE:
        case DX_IDX_EMPTY:     fprintf(stderr, "Line %llu: %s line is too long (> %d chars)\n", (unsigned long long) line,
                                       tool == TOOL_DEXAR && line != 1 ? "Fasta" : t->what, 99998); break;   /* dexta.c:110,168; dexar.c says "Arrow" for line 1
                                                                                                                 (dexar.c:109) and "Fasta" for every other (dexar.c:175) */
        case DX_IDX_NO_HEADER: fprintf(stderr, "Line 1: First header in %s file is missing\n", tool == TOOL_DEXTA ? "fasta" : "arrow"); break;   /* dexta.c:114 */
        default:               fprintf(stderr, "%s: Header line incorrectly formatted ?\n", Prog); break;                                        /* dexta.c:120,148,154 */
      }
}

/* ---- one file --------------------------------------------------------------------------------- */

typedef struct { int tool, verbose, keep, pipe, upper, lossy, width; } options;

/* one file's way through a tool */
typedef struct
  { char    *pwd, *root, *src, *dst;         /* names (with -i: root alone) */
    FILE    *input, *output;
    int      out_fd, seek;                   /* seek: the output was written at its offsets, the stream's position is still to follow */
    uint8_t *in;  size_t n;  int mapped;     /* the whole input, once read_input has run, and how unslurp releases it */
    uint8_t  key[2];  size_t nkey;           /* the input's first bytes (an image's endian key, for the reference's words about a wrong one) */
    dx_ctx  *ctx;                            /* the context the route took */
    size_t   out_len;
    uint64_t line;  int code;                /* where and why a text is malformed (DX_E_FORMAT) */
  } job;

/* DEXGPU_TIMING=1: wall-clock marks on stderr (where an end-to-end run spends its time) */
static void tmark(const char *what)
{ static double t0 = -1.0;
  struct timespec ts;
  double now;
  if (getenv("DEXGPU_TIMING") == NULL) return;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  now = ts.tv_sec + 1e-9 * ts.tv_nsec;
  if (t0 < 0) t0 = now;
  fprintf(stderr, "[%s %8.1f ms] %s\n", Prog, (now - t0) * 1e3, what);
}

/* ---- the GPU contexts --------------------------------------------------------------------------- */

/* They are opened on a second thread while the first input file is being read
   (HIP initialisation and a large read each take a few hundred milliseconds). */
static dx_ctx *Ctxs[64];     /* DEXGPU_DEVICES: one context per listed GPU; a file's entries are sharded over them */
static int     Nctx = 0;
static dx_ctx *Ctx0 = NULL;

static void *open_contexts(void *arg)
{ dx_ctx *ctx = NULL;
  int     k;
  const char *dev = getenv("DEXGPU_DEVICE"), *devs = getenv("DEXGPU_DEVICES");
  (void) arg;
  if (devs != NULL && *devs != '\0')              /* "all" or a comma list, e.g. 0,1,2,3 */
    { if (strcmp(devs, "all") == 0)
        { int nd = dx_device_count();
          for (k = 0; k < nd && k < 64; k++)
            if (dx_open(k, &Ctxs[Nctx]) == DX_OK) Nctx += 1;
        }
      else
        { const char *q = devs;
          while (*q != '\0' && Nctx < 64)
            { char *e;
              long  d = strtol(q, &e, 10);
              if (e == q) break;
              if (dx_open((int) d, &Ctxs[Nctx]) != DX_OK)
                { fprintf(stderr, "%s: cannot open GPU %ld: %s\n", Prog, d, dx_last_error(NULL));
                  exit(1);
                }
              Nctx += 1;
              q = (*e == ',') ? e + 1 : e;
            }
        }
      if (Nctx > 0) ctx = Ctxs[0];
    }
  if (ctx == NULL && dx_open(dev ? atoi(dev) : 0, &ctx) != DX_OK)
    { fprintf(stderr, "%s: cannot open a GPU: %s\n", Prog, dx_last_error(NULL));
      exit(1);
    }
  Ctx0 = ctx;
  return NULL;
}

static pthread_t Opener;
static int       Opening = 0;

/* Ctx0, Ctxs and Nctx are the opener's until this has waited for it */
static dx_ctx *opened(void)
{ if (Opening)
    { pthread_join(Opener, NULL);
      Opening = 0;
    }
  return Ctx0;
}

/* leave only after the opener thread is done: exit() while HIP initialises on another thread is unsafe */
static void leave(int code) { (void) opened(); exit(code); }

/* a route takes the context when it has nothing left to do beside the opener */
static dx_ctx *context(void)
{ dx_ctx *ctx = opened();
  tmark("GPU context open");
  return ctx;
}

/* Is there but one context?  Without DEXGPU_DEVICES the opener leaves Ctxs and Nctx alone and the environment says so: the
   opener goes on beside the reading of the input.  With it the count is the opener's to give, so it is waited for first. */
static int one_context(void)
{ const char *devs = getenv("DEXGPU_DEVICES");
  if (devs != NULL && *devs != '\0') (void) opened();
  return Nctx <= 1;
}

/* ---- sinks and sources of the file drivers ------------------------------------------------------ */

/* the output file at its offset */
static int sink_pwrite(void *user, uint8_t *data, size_t len, size_t at)
{ const int fd = *(int *) user;
  size_t done = 0;
  while (done < len)
    { ssize_t k = pwrite(fd, data + done, len - done, (off_t) (at + done));
      if (k <= 0) return 1;
      done += (size_t) k;
    }
  return 0;
}

/* ... sink_pwrite's user for a run's output; the end of the run moves the stream's position behind what was written */
static void *at_offsets(job *f) { f->seek = 1; return &f->out_fd; }

/* a pipe: the chunks come in file order (dx_file_pack2_stream) */
static int sink_stream(void *user, uint8_t *data, size_t len, size_t at)
{ (void) at;
  return fwrite(data, 1, len, (FILE *) user) != len;
}

static int sink_memory(void *user, uint8_t *data, size_t len, size_t at)
{ memcpy((uint8_t *) user + at, data, len);
  return 0;
}

/* dx_read_fn over a descriptor: a pipe gives what it has, so ask until the want is met or the input ends */
static long read_fd(void *user, void *buf, size_t want)
{ const int fd = *(int *) user;
  size_t got = 0;
  while (got < want)
    { const ssize_t k = read(fd, (uint8_t *) buf + got, want - got);
      if (k < 0) return -1;
      if (k == 0) break;
      got += (size_t) k;
    }
  return (long) got;
}

/* ... with the input's first bytes looked at beforehand (a job's key) */
typedef struct { int fd; const uint8_t *pre; size_t npre, given; } peek_fd;
static long read_peeked(void *user, void *buf, size_t want)
{ peek_fd *p = user;
  size_t got = 0;
  while (p->given < p->npre && got < want) ((uint8_t *) buf)[got++] = p->pre[p->given++];
  if (got < want)
    { const long k = read_fd(&p->fd, (uint8_t *) buf + got, want - got);
      if (k < 0) return -1;
      got += (size_t) k;
    }
  return (long) got;
}

/* ... and a large output file whose size is known (undexqv: the plan's) or can be guessed (dexqv: three tenths of the text):
   a helper thread allocates its pages a stretch at a time while the text is still on its way -- one posix_fallocate call for
   20 GB takes a second during which nothing else goes on --, and the sink writes a chunk (pwrite, in order, one thread) as soon
   as the pages under it are there; what the guess leaves out the write allocates itself, what it has too much ftruncate takes
   back.  For dexqv, whose output is ready while its pages can still be laid out beside the upload (5.7 GB: 0.93 -> 0.49 s).
   (Measured and not kept for undexqv's 20 GB of text: the chunks copied into a shared mapping of the file by six threads -- every
   page of the mapping faults once: 3.1 s where one thread's pwrite takes 2.0, and several threads' pwrite queue up behind the
   inode's lock; the allocator beside the writer -- the two take turns at that lock: 2.1 - 4.5 s; the file allocated whole, then
   written, is what undexqv does: 0.9 + 2.0 s.)  A full file system is an error return of posix_fallocate or pwrite.       */
#define OUT_STRETCH ((size_t) 256 << 20)
typedef struct
  { size_t n; int fd; size_t upto;
    pthread_mutex_t mx; pthread_cond_t cv; pthread_t th; int threaded;
  } outfile;

static void *outfile_alloc(void *arg)
{ outfile *o = arg;
  size_t off;
  for (off = 0; off < o->n; off += OUT_STRETCH)
    { const size_t len = o->n - off < OUT_STRETCH ? o->n - off : OUT_STRETCH;
      /* The size is a guess and laying pages out ahead is a convenience: when the file system will not (ENOSPC on an
         over-estimate, EOPNOTSUPP / EINVAL where there is no fallocate) the writer simply goes on without -- pwrite
         reports what is really wrong with the output, if anything is.                                             */
      const int bad = posix_fallocate(o->fd, (off_t) off, (off_t) len) != 0;
      pthread_mutex_lock(&o->mx);
      o->upto = bad ? o->n : off + len;
      pthread_cond_broadcast(&o->cv);
      pthread_mutex_unlock(&o->mx);
      if (bad) break;
    }
  return NULL;
}

static int outfile_begin(outfile *o, FILE *f, size_t expect)
{ memset(o, 0, sizeof(*o));
  o->fd = fileno(f); o->n = expect;
  { const size_t least = (size_t) dx_test_num("outfile_min", (long long) 1 << 30);          /* (tests: that way from this size on) */
    if (expect < least || expect == 0 || !file_is_ours(f)) return 0;
  }
  pthread_mutex_init(&o->mx, NULL);
  pthread_cond_init(&o->cv, NULL);
  o->threaded = pthread_create(&o->th, NULL, outfile_alloc, o) == 0;
  if (!o->threaded) (void) outfile_alloc(o);
  return 1;
}

static int sink_outfile(void *user, uint8_t *data, size_t len, size_t at)
{ outfile *o = user;
  const size_t want = at + len < o->n ? at + len : o->n;    /* (behind the expected size: the write allocates) */
  pthread_mutex_lock(&o->mx);
  while (o->upto < want) pthread_cond_wait(&o->cv, &o->mx);
  pthread_mutex_unlock(&o->mx);
  return sink_pwrite(&o->fd, data, len, at);
}

static int outfile_end(outfile *o, size_t size)             /* 0: the file is complete, `size` bytes long */
{ if (o->threaded) pthread_join(o->th, NULL);
  pthread_cond_destroy(&o->cv);
  pthread_mutex_destroy(&o->mx);
  return ftruncate(o->fd, (off_t) size) != 0 || lseek(o->fd, (off_t) size, SEEK_SET) < 0;
}

/* ---- the routes, in the order they are asked ---------------------------------------------------- */

/* A route's answer when its precondition does not hold: the next one is asked (as after DX_E_AGAIN, a driver's own "not this way"). */
#define NOT_MINE 1

/* the size of a regular file, -1 of anything else */
static off_t file_size(FILE *f)
{ struct stat st;
  return fstat(fileno(f), &st) == 0 && S_ISREG(st.st_mode) ? st.st_size : -1;
}

static int letters(const options *o) { return o->tool == TOOL_UNDEXAR ? DX_LETTERS_ARROW : (o->upper ? DX_LETTERS_UPPER : DX_LETTERS_LOWER); }

/* 1. A large .quiva is read from its file straight into the buffers that go to the GPU (dx_file_dexqv_fd_to): no image of it in
   this process, whose pages a mapping brings in one by one and gives back one by one (a second and a half of the two and a half
   a 20 GB file took).  DX_E_AGAIN: the driver wants it in memory after all. */
static int dexqv_from_descriptor(const options *o, job *f)
{ const off_t size = file_size(f->input);
  outfile of;
  int rc;
  if (o->tool != TOOL_DEXQV || o->pipe || !one_context() || size <= 0 ||
      size < (off_t) dx_test_num("fd_min", (long long) 256 << 20) || !file_is_ours(f->output))       /* (tests: that way from this size on) */
    return NOT_MINE;
  f->ctx = context();
  if (!outfile_begin(&of, f->output, (size_t) size / 10 * 3))                                          /* (a .dexqv is about three tenths of its .quiva) */
    return dx_file_dexqv_fd_to(f->ctx, fileno(f->input), (size_t) size, o->lossy, sink_pwrite, at_offsets(f), &f->out_len, &f->line, &f->code);
  rc = dx_file_dexqv_fd_to(f->ctx, fileno(f->input), (size_t) size, o->lossy, sink_outfile, &of, &f->out_len, &f->line, &f->code);
  if (outfile_end(&of, rc == DX_OK ? f->out_len : 0) && rc == DX_OK) rc = DX_E_IO;
  return rc;
}

/* 2. dexta -i / dexar -i, and a file too large to hold beside its image (8 GiB and more): the text goes through the device a chunk
   of whole records at a time (dx_file_pack2_stream) -- as the reference reads record after record (dexta.c:104-205), with a
   chunk's memory whatever the input's size.  (Smaller files stay whole: a mapping, one upload, one pass -- 0.9 s for 4 GB where
   the pieces, one after the other, take 1.6.) */
static int pack2_streamed(const options *o, job *f)
{ const off_t size = file_size(f->input);
  int fdin = fileno(f->input);
  if ((o->tool != TOOL_DEXTA && o->tool != TOOL_DEXAR) || !one_context() ||
      !(o->pipe || (size >= 0 && size >= (off_t) dx_test_num("fd_min", (long long) 8 << 30) && file_is_ours(f->output))))
    return NOT_MINE;
  f->ctx = context();
  if (o->pipe || !file_is_ours(f->output))          /* (a pipe: 64 MiB at a time -- the memory stays small, the pipe sets the pace) */
    return dx_file_pack2_stream(f->ctx, o->tool == TOOL_DEXAR, read_fd, &fdin, (size_t) dx_test_num("stream_chunk", (long long) 64 << 20),
                                sink_stream, f->output, &f->out_len, &f->line, &f->code);
  return dx_file_pack2_stream(f->ctx, o->tool == TOOL_DEXAR, read_fd, &fdin, 0, sink_pwrite, at_offsets(f), &f->out_len, &f->line, &f->code);
}

/* 3. undexta -i / undexar -i: the image through the device a chunk of whole records at a time, their text out in order
   (the reference reads and writes record after record, undexta.c:175-271) */
static int unpack2_streamed(const options *o, job *f)
{ peek_fd pk = { fileno(f->input), f->key, 0, 0 };
  long k;
  if ((o->tool != TOOL_UNDEXTA && o->tool != TOOL_UNDEXAR) || !o->pipe) return NOT_MINE;
  k = read_fd(&pk.fd, f->key, 2);
  pk.npre = f->nkey = k > 0 ? (size_t) k : 0;
  f->ctx = context();
  return dx_file_unpack2_stream(f->ctx, letters(o), read_peeked, &pk, 0, (uint32_t) o->width, sink_stream, f->output, &f->out_len);
}

/* Every route behind this one has the whole input before it. */
static int read_input(const options *o, job *f)
{ (void) o;
  f->in = slurp(f->input, &f->n, &f->mapped);
  tmark("input read");
  f->nkey = f->in == NULL ? 0 : (f->n < 2 ? f->n : 2);
  if (f->nkey > 0) memcpy(f->key, f->in, f->nkey);
  return NOT_MINE;
}

/* 4. undexqv: the text goes from the GPU into the output file chunk by chunk (no image of it in this process): its size comes
   from the host walk over the record stream, which runs while the GPU context is still being opened, and so does the
   allocation of the file's pages. */
static int undexqv_by_plan(const options *o, job *f)
{ dx_undexqv_plan *plan = NULL;
  int rc;
  if (o->tool != TOOL_UNDEXQV || f->in == NULL || !one_context()) return NOT_MINE;
  if (f->n >= ((size_t) 256 << 20))                  /* a large file: its records are walked on the GPU (dx_file_undexqv_plan_on) */
    rc = dx_file_undexqv_plan_on(f->ctx = opened(), f->in, f->n, &plan, &f->out_len);
  else
    rc = dx_file_undexqv_plan(f->in, f->n, &plan, &f->out_len);
  tmark("records walked");
  if (rc != DX_OK) return rc;
  { const int direct = file_is_ours(f->output) && (f->out_len == 0 || posix_fallocate(f->out_fd, 0, (off_t) f->out_len) == 0) &&
                       ftruncate(f->out_fd, (off_t) f->out_len) == 0;
    tmark("output file allocated");
    f->ctx = context();
    if (direct)
      rc = dx_file_undexqv_run(f->ctx, plan, o->upper, sink_pwrite, at_offsets(f));
    else                                             /* a pipe: through memory */
      { uint8_t *out = malloc(f->out_len + 16);
        rc = out == NULL ? DX_E_NOMEM : dx_file_undexqv_run(f->ctx, plan, o->upper, sink_memory, out);
        if (rc == DX_OK && f->out_len > 0 && fwrite(out, 1, f->out_len, f->output) != f->out_len) rc = DX_E_IO;
        free(out);
      }
  }
  dx_file_undexqv_plan_free(plan);
  return rc;
}

/* 5. dexqv on one context, undexta, undexar: the output goes from the GPU into the output file chunk by chunk, if that is a
   regular file of ours */
static int into_our_file(const options *o, job *f)
{ const int qv = o->tool == TOOL_DEXQV;
  if (f->in == NULL || !(qv ? one_context() : (o->tool == TOOL_UNDEXTA || o->tool == TOOL_UNDEXAR)) || !file_is_ours(f->output))
    return NOT_MINE;
  f->ctx = context();
  if (qv)
    return dx_file_dexqv_to(f->ctx, f->in, f->n, o->lossy, sink_pwrite, at_offsets(f), &f->out_len, &f->line, &f->code);
  return dx_file_unpack2_to(f->ctx, letters(o), f->in, f->n, (uint32_t) o->width, sink_pwrite, at_offsets(f), &f->out_len);
}

/* 6. Everything else -- a file over several contexts among it -- is converted whole in memory and its image written whole. */
static int whole_in_memory(const options *o, job *f)
{ uint8_t *out = NULL;
  int rc;
  f->ctx = context();
  if (f->in == NULL)
    { fprintf(stderr, "%s: Out of memory (Allocating read buffer)\n", Prog);
      leave(1);
    }
  if (o->tool == TOOL_DEXQV && Nctx > 1)
    rc = dx_file_dexqv_sharded(Ctxs, Nctx, f->in, f->n, o->lossy, &out, &f->out_len, &f->line, &f->code);
  else if ((o->tool == TOOL_DEXTA || o->tool == TOOL_DEXAR) && Nctx > 1)
    rc = dx_file_pack2_sharded(Ctxs, Nctx, o->tool == TOOL_DEXAR, f->in, f->n, &out, &f->out_len, &f->line, &f->code);
  else if (o->tool == TOOL_DEXTA || o->tool == TOOL_DEXAR)
    rc = dx_file_pack2(f->ctx, o->tool == TOOL_DEXAR, f->in, f->n, &out, &f->out_len, &f->line, &f->code);
  else if (o->tool == TOOL_DEXQV)
    rc = dx_file_dexqv(f->ctx, f->in, f->n, o->lossy, &out, &f->out_len, &f->line, &f->code);
  else if (o->tool == TOOL_UNDEXQV)
    rc = dx_file_undexqv(f->ctx, f->in, f->n, o->upper, &out, &f->out_len);
  else
    rc = dx_file_unpack2(f->ctx, letters(o), f->in, f->n, (uint32_t) o->width, &out, &f->out_len);
  if (rc != DX_OK) return rc;
  tmark("converted (index, copies, kernels)");
  if (write_image(f->output, out, f->out_len) != 0) rc = DX_E_IO;
  dx_file_free(out);
  return rc;
}

static int (*const ROUTES[])(const options *, job *) =
  { dexqv_from_descriptor, pack2_streamed, unpack2_streamed, read_input, undexqv_by_plan, into_our_file, whole_in_memory };

/* ---- a file's beginning and end ----------------------------------------------------------------- */

/* a route's failure in the reference's words; the exit status */
static int report_failure(int tool, const job *f, int rc)
{ if (rc == DX_E_IO)
    { fprintf(stderr, "%s: System error, write failed!\n", Prog);
      return 2;
    }
  if (rc == DX_E_FORMAT && (tool == TOOL_DEXTA || tool == TOOL_DEXAR || tool == TOOL_DEXQV))
    { report_text_error(tool, f->line, f->code);
      return 1;
    }
  if (rc == DX_E_FORMAT && f->nkey >= 2 && (tool == TOOL_UNDEXTA || tool == TOOL_UNDEXAR))
    { uint16_t key;
      memcpy(&key, f->key, 2);
      if (key != 0x55aa && key != 0xaa55 && !(tool == TOOL_UNDEXTA && (key == 0x33cc || key == 0xcc33)))
        { fprintf(stderr, "%s: Not a .%s file, endian key invalid\n", Prog, TOOLS[tool].what);   /* undexta.c:156 */
          return 1;
        }
    }
  if (rc == DX_E_FORMAT)
    { fprintf(stderr, "%s: System error, read failed!\n", Prog);                                 /* DB.h:136-139 */
      return 2;
    }
  { const char *why = dx_last_error(f->ctx);
    if (why == NULL || why[0] == '\0')                    /* (host-side failures carry a code only) */
      why = rc == DX_E_DEGENERATE ? "a stream that needs a Huffman scheme holds no symbols (e.g. a deletion line of nothing but its run "
                                    "character, or an empty file): the reference reads out of bounds there (QV.c:201), nothing is written"
          : rc == DX_E_NOMEM      ? "out of memory"
          : rc == DX_E_UNSUPPORTED ? "a code longer than 16 bits: the reference would write a file its own decoder cannot read"
          : "failed";
    fprintf(stderr, "%s: %s (libdexgpu error %d)\n", Prog, why, rc);
  }
  return 1;
}

/* DEXGPU_VERIFY=1 (dexta, dexar, dexqv of a file): before the source goes, is it what the file just written gives back?  Both as
   they are on disk now, decoded and compared on the GPU (dx_file_verify).  1: yes -- with -v, the invocation that restores it. */
static int verified_on_disk(dx_ctx *ctx, int tool, const char *src, const char *dst, int lossy, int verbose)
{ static const char *where[] = { "nothing", "header line", "body", "body length", "record count", "image" };
  const int kind = tool == TOOL_DEXTA ? DX_KIND_FASTA : (tool == TOOL_DEXAR ? DX_KIND_ARROW : DX_KIND_QUIVA);
  FILE    *fs = fopen(src, "r"), *fd = fopen(dst, "r");
  uint8_t *text = NULL, *img = NULL;
  size_t   n = 0, m = 0;
  int      tmapped = 0, imapped = 0, rc = DX_E_IO, ok = 0;
  dx_verify_report rep;
  memset(&rep, 0, sizeof(rep));
  if (fs != NULL && fd != NULL && (text = slurp(fs, &n, &tmapped)) != NULL && (img = slurp(fd, &m, &imapped)) != NULL)
    rc = dx_file_verify(ctx, kind, text, n, img, m, lossy, &rep);
  if (rc != DX_OK)
    fprintf(stderr, "%s: %s could not be verified against %s (%s); both are kept\n", Prog, dst, src,
            rc == DX_E_IO ? "cannot be read" : dx_last_error(ctx));
  else if (!rep.ok)
    fprintf(stderr, "%s: %s does not give %s back: record %llu, line %llu, column %llu (%s); both are kept\n", Prog, dst, src,
            (unsigned long long) rep.record, (unsigned long long) rep.line, (unsigned long long) rep.column, where[rep.where]);
  else
    { ok = 1;
      if (verbose)
        { if (kind == DX_KIND_QUIVA) fprintf(stderr, "Verified (undexqv%s)\n", rep.upper ? " -U" : "");
          else fprintf(stderr, "Verified (%s%s -w%u)\n", kind == DX_KIND_ARROW ? "undexar" : "undexta", rep.upper ? " -U" : "", rep.width);
        }
    }
  if (text != NULL) unslurp(text, n, tmapped);
  if (img != NULL) unslurp(img, m, imapped);
  if (fs != NULL) fclose(fs);
  if (fd != NULL) fclose(fd);
  return ok;
}

/* DEXGPU_DIGEST: the CRC-32 (zlib's) and the size of the text behind a file's image -- of what the undex* tool makes of it with its -U
   and -w, never assembled: dx_file_digest decodes and hashes on the GPU.  undexta, undexar, undexqv: the image is the input in memory;
   dexta, dexar, dexqv: the image just written, as it is on disk, with the options read off the source as DEXGPU_VERIFY reads them
   (dx_file_text_options) -- what undex* gives back, which DEXGPU_VERIFY=1 says is the source. */
static int is_undex(int tool) { return tool == TOOL_UNDEXTA || tool == TOOL_UNDEXAR || tool == TOOL_UNDEXQV; }

static int digest_of(const options *o, job *f, dx_digest *dg)
{ const int kind = o->tool == TOOL_DEXTA || o->tool == TOOL_UNDEXTA ? DX_KIND_FASTA
                 : (o->tool == TOOL_DEXAR || o->tool == TOOL_UNDEXAR ? DX_KIND_ARROW : DX_KIND_QUIVA);
  int      upper = o->upper, rc = DX_OK;
  uint32_t width = (uint32_t) o->width;
  if (f->ctx == NULL) f->ctx = context();
  if (is_undex(o->tool))
    return f->in == NULL ? DX_E_NOMEM : dx_file_digest(f->ctx, kind, f->in, f->n, upper, width, dg, NULL);
  { FILE    *fs = fopen(f->src, "r"), *fd = fopen(f->dst, "r");
    uint8_t *text = NULL, *img = NULL;
    size_t   n = 0, m = 0;
    int      tmapped = 0, imapped = 0;
    if (fs == NULL || fd == NULL || (text = slurp(fs, &n, &tmapped)) == NULL || (img = slurp(fd, &m, &imapped)) == NULL) rc = DX_E_IO;
    if (rc == DX_OK) rc = dx_file_text_options(kind, text, n, &upper, &width);
    if (text != NULL) unslurp(text, n, tmapped);
    if (rc == DX_OK) rc = dx_file_digest(f->ctx, kind, img, m, upper, width ? width : 1, dg, NULL);
    if (img != NULL) unslurp(img, m, imapped);
    if (fs != NULL) fclose(fs);
    if (fd != NULL) fclose(fd);
  }
  return rc;
}

/* DEXGPU_CENSUS: what the image holds (dx_file_census: counted on the GPU where it lies or is decoded to, no text made or downloaded), on
   one line: records, symbols, the shortest and the longest read, N50, then the symbols code by code (fasta, arrow) or the mean byte value
   of the deletion, insertion, merge and substitution QV lines (quiva).  The image is the one DEXGPU_DIGEST takes. */
static int census_of(const options *o, job *f, dx_census *cs)
{ const int kind = o->tool == TOOL_DEXTA || o->tool == TOOL_UNDEXTA ? DX_KIND_FASTA
                 : (o->tool == TOOL_DEXAR || o->tool == TOOL_UNDEXAR ? DX_KIND_ARROW : DX_KIND_QUIVA);
  int rc = DX_OK;
  if (f->ctx == NULL) f->ctx = context();
  if (is_undex(o->tool))
    return f->in == NULL ? DX_E_NOMEM : dx_file_census(f->ctx, kind, f->in, f->n, cs, NULL, NULL, NULL);
  { FILE    *fd = fopen(f->dst, "r");
    uint8_t *img = NULL;
    size_t   m = 0;
    int      imapped = 0;
    if (fd == NULL || (img = slurp(fd, &m, &imapped)) == NULL) rc = DX_E_IO;
    if (rc == DX_OK) rc = dx_file_census(f->ctx, kind, img, m, cs, NULL, NULL, NULL);
    if (img != NULL) unslurp(img, m, imapped);
    if (fd != NULL) fclose(fd);
  }
  return rc;
}

static void census_line(const options *o, const dx_census *cs, const char *path)
{ printf("records=%llu symbols=%llu min=%u max=%u n50=%u", (unsigned long long) cs->records, (unsigned long long) cs->symbols,
         cs->min_len, cs->max_len, cs->n50);
  if (o->tool == TOOL_DEXQV || o->tool == TOOL_UNDEXQV)
    { static const char *name[4] = { "del", "ins", "mrg", "sub" };
      static const int   line[4] = { 0, 2, 3, 4 };
      int q, v;
      for (q = 0; q < 4; q++)
        { double sum = 0.0;
          for (v = 0; v < 256; v++) sum += (double) v * (double) cs->hist[line[q]][v];
          printf(" %s=%.3f", name[q], cs->symbols ? sum / (double) cs->symbols : 0.0);
        }
    }
  else
    { const char *name = o->tool == TOOL_DEXTA || o->tool == TOOL_UNDEXTA ? "acgt" : "1234";
      int q;
      for (q = 0; q < 4; q++) printf(" %c=%llu", name[q], (unsigned long long) cs->code[q]);
    }
  printf(" %s\n", path);
  fflush(stdout);
}

/* the files behind a name (dexta.c:87-94), or the standard streams */
static void begin(const options *o, const char *name, job *f)
{ const tool_t *t = &TOOLS[o->tool];
  memset(f, 0, sizeof(*f));
  if (o->pipe)
    { f->input  = stdin;
      f->output = stdout;
      f->root   = strdup("Standard Input");
    }
  else
    { f->pwd  = path_to(name);
      f->root = root_of(name, t->src_ext);
      f->src  = catenate(f->pwd, f->root, t->src_ext);
      f->dst  = catenate(f->pwd, f->root, t->dst_ext);
      if ((f->input = fopen(f->src, "r")) == NULL)
        { fprintf(stderr, "%s: Cannot open %s for 'r'\n", Prog, f->src);   /* Fopen, DB.c:103-110 */
          leave(1);
        }
      if (!LINES_ONLY && (f->output = fopen(f->dst, "w+")) == NULL)     /* (readable too: a large output is written through a shared mapping, which wants that) */
        { fprintf(stderr, "%s: Cannot open %s for 'w'\n", Prog, f->dst);
          leave(1);
        }
    }
  f->out_fd = f->output != NULL ? fileno(f->output) : -1;       /* (DEXGPU_DIGEST=only, DEXGPU_CENSUS=only: there is no output) */
  if (o->verbose)
    { fprintf(stderr, "Processing '%s' ...\n", f->root);
      fflush(stderr);
    }
}

/* The one end of a file's run, whichever route it took and whatever that answered. */
static void end(const options *o, job *f, int rc)
{ dx_digest  dg;
  dx_census *cs = NULL;
  memset(&dg, 0, sizeof(dg));
  if (Census && (cs = calloc(1, sizeof(*cs))) == NULL) rc = rc == DX_OK ? DX_E_NOMEM : rc;
  if (rc == DX_OK && f->seek && lseek(f->out_fd, (off_t) f->out_len, SEEK_SET) < 0) rc = DX_E_IO;
  if (rc == DX_OK && Digest && is_undex(o->tool))          /* (the image is the input, while it is still in memory) */
    { rc = digest_of(o, f, &dg);
      tmark("digested");
    }
  if (rc == DX_OK && Census && is_undex(o->tool))
    { rc = census_of(o, f, cs);
      tmark("counted");
    }
  if (rc == DX_OK)
    { if (f->in != NULL) unslurp(f->in, f->n, f->mapped);
      tmark("output written");
      if (!o->pipe) fclose(f->input);
      if (f->output != NULL && (o->pipe ? fflush(f->output) != 0 : fclose(f->output) != 0))   /* a deferred write error (ENOSPC, quota, NFS) */
        rc = DX_E_IO;                                                                         /* surfaces here: the source must survive it */
    }
  if (rc != DX_OK)
    leave(report_failure(o->tool, f, rc));
  if (Digest && !is_undex(o->tool))                        /* (the image is the file just closed) */
    { if ((rc = digest_of(o, f, &dg)) != DX_OK)
        { fprintf(stderr, "%s: %s could not be digested (%s); %s is kept\n", Prog, f->dst,
                  rc == DX_E_IO ? "cannot be read" : dx_last_error(f->ctx), f->src);
          leave(1);
        }
      tmark("digested");
    }
  if (Census && !is_undex(o->tool))
    { if ((rc = census_of(o, f, cs)) != DX_OK)
        { fprintf(stderr, "%s: %s could not be counted (%s); %s is kept\n", Prog, f->dst,
                  rc == DX_E_IO ? "cannot be read" : dx_last_error(f->ctx), f->src);
          leave(1);
        }
      tmark("counted");
    }
  if (Digest)
    { printf("%08x %llu %s\n", dg.crc32, (unsigned long long) dg.bytes, is_undex(o->tool) ? f->dst : f->src);
      fflush(stdout);
    }
  if (Census)
    { census_line(o, cs, is_undex(o->tool) ? f->dst : f->src);
      free(cs);
    }
  if (!o->pipe)
    { const char *verify = getenv("DEXGPU_VERIFY");
      if ((o->tool == TOOL_DEXTA || o->tool == TOOL_DEXAR || o->tool == TOOL_DEXQV) && verify != NULL && atoi(verify) != 0)
        { if (!verified_on_disk(f->ctx, o->tool, f->src, f->dst, o->lossy, o->verbose))
            leave(3);                                    /* (the reference's tools leave with 1 and 2; the files that follow are not touched) */
          tmark("verified");
        }
      if (!o->keep && !LINES_ONLY) unlink(f->src);           /* (DEXGPU_DIGEST=only, DEXGPU_CENSUS=only made nothing that could stand in for it) */
    }
  free(f->root); free(f->pwd); free(f->src); free(f->dst);
  if (o->verbose)
    { fprintf(stderr, "Done\n");
      fflush(stderr);
    }
}

/* ---- the tool ----------------------------------------------------------------------------------- */

/* The options and, in argv[1..], the file names; the number of both is returned.  Argument errors leave here, in the reference's
   words, before any thread is started. */
static int parse_arguments(int tool, int argc, char *argv[], options *o)
{ const tool_t *t = &TOOLS[tool];
  int flags[128], i, j, k;

  memset(flags, 0, sizeof(flags));
  memset(o, 0, sizeof(*o));
  o->tool  = tool;
  o->width = 80;

  j = 1;                                                   /* ARG_INIT / ARG_FLAGS, DB.h:79-91 */
  for (i = 1; i < argc; i++)
    if (argv[i][0] == '-')
      { if (argv[i][1] == 'w' && (tool == TOOL_UNDEXTA || tool == TOOL_UNDEXAR))
          { char *eptr;                                    /* ARG_NON_NEGATIVE, DB.h:105-115 */
            o->width = (int) strtol(argv[i] + 2, &eptr, 10);
            if (*eptr != '\0' || argv[i][2] == '\0')
              { fprintf(stderr, "%s: -%c '%s' argument is not an integer\n", Prog, argv[i][1], argv[i] + 2);
                exit(1);
              }
            if (o->width < 0)
              { fprintf(stderr, "%s: %s must be non-negative (%d)\n", Prog, "Line width", o->width);
                exit(1);
              }
            continue;
          }
        for (k = 1; argv[i][k] != '\0'; k++)
          { if (strchr(t->flags, argv[i][k]) == NULL)
              { fprintf(stderr, "%s: -%c is an illegal option\n", Prog, argv[i][k]);
                exit(1);
              }
            flags[(int) argv[i][k]] = 1;
          }
      }
    else
      argv[j++] = argv[i];
  argc = j;

  o->verbose = flags['v'];
  o->pipe    = flags['i'];
  o->keep    = flags['k'] || o->pipe;
  o->upper   = flags['U'];
  o->lossy   = flags['l'];

  if ((t->pipe_ok && ((o->pipe && argc > 1) || (!o->pipe && argc <= 1))) || (!t->pipe_ok && argc == 1))
    { fprintf(stderr, "Usage: %s %s\n", Prog, t->usage);   /* e.g. dexta.c:47-54 */
      fprintf(stderr, "\n");
      for (k = 0; k < 4; k++)
        if (t->help[k] != NULL)
          fprintf(stderr, "%s", t->help[k]);
      exit(1);
    }
  if (o->width == 0)
    { fprintf(stderr, "%s: Line width must be positive (the reference never terminates on -w0)\n", Prog);
      exit(1);
    }
  return o->pipe ? 2 : argc;                               /* (-i: one run, on the standard streams) */
}

int dex_tool_main(int tool, int argc, char *argv[])
{ options o;
  int     i, k;

  Prog = TOOLS[tool].name;
  argc = parse_arguments(tool, argc, argv, &o);

  { const char *d = getenv("DEXGPU_DIGEST");              /* (with -i stdout carries the data: no line there) */
    Digest = d == NULL || *d == '\0' || o.pipe ? 0 : (strcmp(d, "only") == 0 ? 2 : atoi(d) != 0);
    if (Digest == 2 && !is_undex(tool))
      { fprintf(stderr, "%s: DEXGPU_DIGEST=only digests an image and writes nothing: that is for un%s; %s is there to write one\n",
                Prog, Prog, Prog);
        exit(1);
      }
  }
  { const char *d = getenv("DEXGPU_CENSUS");              /* (the same rules) */
    Census = d == NULL || *d == '\0' || o.pipe ? 0 : (strcmp(d, "only") == 0 ? 2 : atoi(d) != 0);
    if (Census == 2 && !is_undex(tool))
      { fprintf(stderr, "%s: DEXGPU_CENSUS=only counts what an image holds and writes nothing: that is for un%s; %s is there to write one\n",
                Prog, Prog, Prog);
        exit(1);
      }
  }

  tmark("start");
#ifdef F_SETPIPE_SZ
  if (o.pipe) (void) fcntl(0, F_SETPIPE_SZ, 1 << 20);      /* (a pipe's 64 KB are 2 GB/s at best; no harm where stdin is none or the size is refused) */
#endif
  Opening = pthread_create(&Opener, NULL, open_contexts, NULL) == 0;
  if (!Opening) open_contexts(NULL);
  for (i = 1; i < argc; i++)
    { job    f;
      int    rc = NOT_MINE;
      size_t r;
      begin(&o, argv[i], &f);
      if (LINES_ONLY) rc = read_input(&o, &f) == NOT_MINE ? DX_OK : DX_E_IO;     /* (no route: nothing is converted) */
      for (r = 0; r < sizeof(ROUTES) / sizeof(ROUTES[0]) && (rc == NOT_MINE || rc == DX_E_AGAIN); r++)
        { f.seek = 0;                                      /* (what a route that passed the file on has set) */
          rc = ROUTES[r](&o, &f);
        }
      end(&o, &f, rc);
    }

  /* Every output is closed (fclose has reported what there was to report), every input is released: nothing is left but to give
     back what the process holds on the device and in the HIP runtime -- 0.2 s of a 0.45 s run on a 1 GB file (r03c_cli_timing),
     which the system does by itself when the process ends.  DEXGPU_TEARDOWN=1: the orderly way (leak checkers).               */
  (void) opened();                                         /* (never while HIP comes up on another thread) */
  if (getenv("DEXGPU_TEARDOWN") == NULL && getenv("LD_PRELOAD") == NULL && getenv("ROCP_TOOL_LIBRARIES") == NULL &&
      getenv("ROCPROFILER_REGISTER_ROOT") == NULL)        /* (a profiler, a sanitizer or a coverage run writes its output at exit) */
    { tmark("leaving");
      fflush(NULL);
      _exit(0);
    }
  if (Nctx > 0)
    for (k = 0; k < Nctx; k++) dx_close(Ctxs[k]);
  else
    dx_close(Ctx0);
  exit(0);
}
