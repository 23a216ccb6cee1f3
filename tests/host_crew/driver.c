/* The thread crew of csrc/dx_crew.c on its own, under ThreadSanitizer: crews of 1, 2, 5 and 8 walk a table of five phases that has
   all three shapes (work + fold, work only, fold only).  Every member writes its slot in a work phase, member 0 sums the slots in the
   fold and publishes the sum, every member checks what was published in the next work phase -- with nothing but the crew's barriers
   between them, so a barrier too few is a race for the sanitizer and a wrong sum here.  One run has a member mark itself failed in
   the first phase: it walks every phase like the others. */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dx_crew.h"

#define NPHASES 5
#define NSUMS   3

typedef struct shared shared;

typedef struct
  { shared   *sh;
    int       id, fails;                     /* fails: this member is to mark itself failed in the first phase */
    int       failed;
    long      slot;
    int       ran[NPHASES + 1], nran;        /* the phases whose work ran here, in the order they ran */
    int       wrong;                         /* a published value that was not the expected one */
    pthread_t self;
  } member;

struct shared
  { int       n;
    member   *m;
    long      sum[NSUMS];                    /* published by the folds */
    int       nfailed;
    int       folded[NPHASES + 1], nfolded;  /* the phases whose fold ran, in the order they ran */
    int       elsewhere;                     /* a fold that ran on another thread than member 0's */
    pthread_t folder;
  };

static long value(int round, int id) { return round == 0 ? id + 1 : round == 1 ? 10L * (id + 1) : (long) id * id + 7; }

static long expected(int round, int n)
{ long s = 0;
  int  k;
  for (k = 0; k < n; k++) s += value(round, k);
  return s;
}

static void ran(member *m, int phase)
{ if (m->nran <= NPHASES) m->ran[m->nran] = phase;
  m->nran += 1;
}

static void check(member *m, int round)
{ if (m->sh->sum[round] != expected(round, m->sh->n)) m->wrong += 1; }

static void sum_up(shared *sh, int phase, int round)
{ long s = 0;
  int  k;
  if (sh->nfolded <= NPHASES) sh->folded[sh->nfolded] = phase;
  sh->nfolded += 1;
  if (!pthread_equal(pthread_self(), sh->m[0].self)) sh->elsewhere += 1;
  for (k = 0; k < sh->n; k++) s += sh->m[k].slot;
  sh->sum[round] = s;
}

static void work0(void *arg)
{ member *m = arg;
  ran(m, 0);
  m->self = pthread_self();
  if (m->fails) m->failed = 1;
  m->slot = value(0, m->id);
}
static void fold0(void *arg)
{ shared *sh = arg;
  int k;
  sum_up(sh, 0, 0);
  for (k = 0; k < sh->n; k++) sh->nfailed += sh->m[k].failed;
}
static void work1(void *arg)                    /* work only */
{ member *m = arg;
  int k, fails = 0;
  ran(m, 1);
  check(m, 0);
  for (k = 0; k < m->sh->n; k++) fails += m->sh->m[k].fails;
  if (m->sh->nfailed != fails) m->wrong += 1;  /* (the verdict a fold published) */
  m->slot = value(1, m->id);
}
static void fold2(void *arg) { sum_up(arg, 2, 1); }          /* fold only */
static void work3(void *arg)
{ member *m = arg;
  ran(m, 3);
  check(m, 1);
  m->slot = value(2, m->id);
}
static void fold3(void *arg) { sum_up(arg, 3, 2); }
static void work4(void *arg)                    /* work only, and the last step */
{ member *m = arg;
  ran(m, 4);
  check(m, 2);
}

static const dx_crew_phase table[NPHASES] =
  { { work0, fold0 }, { work1, NULL }, { NULL, fold2 }, { work3, fold3 }, { work4, NULL } };

static int run(int n, int failing)
{ static const int works[] = { 0, 1, 3, 4 }, folds[] = { 0, 2, 3 };
  shared  sh;
  member *m = calloc((size_t) n, sizeof(*m));
  int     k, r, bad = 0;
  if (m == NULL) return 1;
  memset(&sh, 0, sizeof(sh));
  sh.n = n; sh.m = m;
  for (k = 0; k < n; k++) { m[k].sh = &sh; m[k].id = k; m[k].fails = k == failing; }
  if (dx_crew_run(n, table, NPHASES, m, sizeof(*m), &sh) != 0) { fprintf(stderr, "crew of %d: not made\n", n); free(m); return 1; }
  for (k = 0; k < n; k++)
    { if (m[k].nran != 4 || memcmp(m[k].ran, works, sizeof(works)) != 0)
        { fprintf(stderr, "crew of %d: member %d ran %d work functions, or not in table order\n", n, k, m[k].nran); bad = 1; }
      if (m[k].wrong)
        { fprintf(stderr, "crew of %d: member %d saw %d wrong published values\n", n, k, m[k].wrong); bad = 1; }
      if (m[k].failed != (k == failing))
        { fprintf(stderr, "crew of %d: member %d failed = %d\n", n, k, m[k].failed); bad = 1; }
    }
  if (sh.nfolded != 3 || memcmp(sh.folded, folds, sizeof(folds)) != 0)
    { fprintf(stderr, "crew of %d: %d folds ran, or not in table order\n", n, sh.nfolded); bad = 1; }
  if (sh.elsewhere)
    { fprintf(stderr, "crew of %d: %d folds ran on another thread than member 0's\n", n, sh.elsewhere); bad = 1; }
  for (r = 0; r < NSUMS; r++)
    if (sh.sum[r] != expected(r, n))
      { fprintf(stderr, "crew of %d: sum %d is %ld, expected %ld\n", n, r, sh.sum[r], expected(r, n)); bad = 1; }
  if (sh.nfailed != (failing >= 0 && failing < n))
    { fprintf(stderr, "crew of %d: %d members seen failed\n", n, sh.nfailed); bad = 1; }
  free(m);
  return bad;
}

int main(void)
{ static const int sizes[] = { 1, 2, 5, 8 };
  int k, bad = 0;
  for (k = 0; k < 4; k++) bad |= run(sizes[k], -1);
  bad |= run(5, 3);                             /* member 3 marks itself failed in the first phase */
  bad |= run(2, 0);                             /* ... and member 0, which folds all the same */
  if (dx_crew_run(0, table, NPHASES, NULL, 0, NULL) == 0) { fprintf(stderr, "a crew of none was made\n"); bad = 1; }
  if (bad) return 1;
  printf("ok\n");
  return 0;
}
