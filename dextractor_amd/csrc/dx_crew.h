/*
 * dx_crew.h -- a crew of host threads that walks one table of phases in step.  Pure pthreads: no dx_* call, no dexgpu.h.
 *
 * A phase is a pair { work, fold }, either of which may be NULL: work(member) runs on every thread, on its own member; fold(shared)
 * runs on member 0's thread alone, after every member's work of that phase.  A barrier stands between any two steps that follow one
 * another, and dx_crew.c is the only place that waits at one: a phase function holds no barrier, so it cannot skip one, whatever
 * way it returns.
 *
 * What a phase function returns to is the crew, which acts on nothing.  The discipline that makes this enough:
 *   - a member writes only its own slot, and only in a work phase: a failure goes into a field of its own (j->rc);
 *   - member 0 reads the others' slots, and writes shared state, only in a fold: there it publishes the verdict (a->ok, a->again)
 *     that the work phases behind it read.
 * Every member walks every phase, whatever the verdict: a work function that has nothing left to do returns at once.
 */
#ifndef DX_CREW_H
#define DX_CREW_H
#include <stddef.h>

typedef struct
  { void (*work)(void *member);
    void (*fold)(void *shared);
  } dx_crew_phase;

/* n threads over phases[0 .. nphases); thread k's member is the k-th of the n slots of member_size bytes at `members`.  The threads
   start behind a gate: all of them exist, or none runs anything.  0: every phase has run; nonzero: the crew could not be made, and
   no phase function has run on any thread. */
__attribute__((visibility("hidden")))
int dx_crew_run(int n, const dx_crew_phase *phases, int nphases, void *members, size_t member_size, void *shared);

#endif
