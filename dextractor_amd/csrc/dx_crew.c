/*
 * dx_crew.c -- the thread crew of dx_crew.h: the start gate, the walk over the phase table, and the one barrier wait of the library.
 */
#include <pthread.h>
#include <stdlib.h>

#include "dx_crew.h"

typedef struct
  { int                  nphases;
    const dx_crew_phase *phases;
    char                *members;
    size_t               member_size;
    void                *shared;
    int                  go;                 /* start gate: 0 wait, 1 run, -1 a thread could not be created: leave */
    pthread_mutex_t      gate_mx;
    pthread_cond_t       gate_cv;
    pthread_barrier_t    bar;
  } crew;

typedef struct { crew *c; int id; } crew_thread;

/* a step (a phase's work, or its fold) begins: every thread has left the step before it.  Nothing precedes the first step, and
   the joins follow the last, so a table of s steps is walked through s - 1 barriers. */
static void next_step(crew *c, int *steps)
{ if ((*steps)++ > 0) pthread_barrier_wait(&c->bar); }

static void *crew_main(void *arg)
{ const crew_thread *t = arg;
  crew *c = t->c;
  void *me = c->members + (size_t) t->id * c->member_size;
  int   go, k, steps = 0;

  pthread_mutex_lock(&c->gate_mx);                        /* all threads exist, or none runs */
  while (c->go == 0) pthread_cond_wait(&c->gate_cv, &c->gate_mx);
  go = c->go;
  pthread_mutex_unlock(&c->gate_mx);
  if (go < 0) return NULL;

  for (k = 0; k < c->nphases; k++)
    { const dx_crew_phase *p = &c->phases[k];
      if (p->work != NULL)
        { next_step(c, &steps);
          p->work(me);
        }
      if (p->fold != NULL)
        { next_step(c, &steps);
          if (t->id == 0) p->fold(c->shared);
        }
    }
  return NULL;
}

int dx_crew_run(int n, const dx_crew_phase *phases, int nphases, void *members, size_t member_size, void *shared)
{ crew         c;
  pthread_t   *th;
  crew_thread *id;
  int          k, started = 0;

  if (n < 1 || nphases < 0) return 1;
  th = calloc((size_t) n, sizeof(*th));
  id = calloc((size_t) n, sizeof(*id));
  if (!th || !id || pthread_barrier_init(&c.bar, NULL, (unsigned) n) != 0)
    { free(th); free(id);
      return 1;
    }
  c.nphases = nphases; c.phases = phases; c.members = members; c.member_size = member_size; c.shared = shared;
  c.go = 0;
  pthread_mutex_init(&c.gate_mx, NULL);
  pthread_cond_init(&c.gate_cv, NULL);
  for (k = 0; k < n; k++)                                 /* the barrier counts n threads: all of them or none */
    { id[k].c = &c; id[k].id = k;
      if (pthread_create(&th[k], NULL, crew_main, &id[k]) != 0) break;
      started += 1;
    }
  pthread_mutex_lock(&c.gate_mx);
  c.go = started == n ? 1 : -1;
  pthread_cond_broadcast(&c.gate_cv);
  pthread_mutex_unlock(&c.gate_mx);
  for (k = 0; k < started; k++)
    pthread_join(th[k], NULL);
  pthread_barrier_destroy(&c.bar);
  pthread_mutex_destroy(&c.gate_mx);
  pthread_cond_destroy(&c.gate_cv);
  free(th); free(id);
  return started == n ? 0 : 1;
}
