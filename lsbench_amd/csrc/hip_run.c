/*
 * What the iteration drivers share on the host ("Host loop"): waiting for the device with a
 * deadline, the loop that feeds it iterations until its state says stop (run_loop), the cache of captured graphs the
 * drivers replay their iterations from, and the rule that sizes a chunk.  PCG (hip_pcg.c), BiCGSTAB, Richardson and the
 * batch of right-hand sides each describe themselves to run_loop in a struct run_loop; GMRES polls once per restart
 * cycle and does not come here.
 */
#define _GNU_SOURCE
#include "hip_solver.h"

#include <sched.h>

/* Sharded solves wait for the device with a deadline: a collective that never
 * completes (a peer process died, ranks disagreeing on the sequence of calls)
 * must end this process with a message and a non-zero exit code, not hang the
 * node until somebody's job limit (opts.comm_deadline_s,
 * LSBENCH_HIP_COMM_DEADLINE_S).  One shard alone simply blocks. */
void wait_event(lsb_hip_solver *sv, hipEvent_t ev, const char *what) {
  if (!sv->multi || !(sv->o.comm_deadline_s > 0.0)) {
    LSB_CHK_HIP(hipEventSynchronize(ev));
    return;
  }
  const double t0 = wall_seconds();
  for (;;) {
    const hipError_t e = hipEventQuery(ev);
    if (e == hipSuccess)
      return;
    if (e != hipErrorNotReady)
      LSB_CHK_HIP(e);
    if (wall_seconds() - t0 > sv->o.comm_deadline_s)
      lsb_give_up("hip_cdna4: %s: the device did not get there within %.0f s -- a collective "
                  "of the sharded solve is hung (rank %d of %d); giving up",
                  what, sv->o.comm_deadline_s, lsb_hip_comm_rank(), lsb_hip_comm_size());
    sched_yield();
  }
}
void drain_stream(lsb_hip_solver *sv, const char *what) {
  if (!sv->multi) {
    LSB_CHK_HIP(hipStreamSynchronize(g_stream));
    return;
  }
  LSB_CHK_HIP(hipEventRecord(sv->ev_poll[0], g_stream));
  wait_event(sv, sv->ev_poll[0], what);
}

/* ---- the chunk rule --------------------------------------------------------------------------------------------
 * Iterations per host poll: about 0.3 ms of device work at an assumed 4 TB/s, an iteration taken for floor_us at the
 * least, within [lo, hi].  An estimate, not a measurement: the poll is pipelined one chunk ahead, so small chunks
 * cost nothing while running, and the size only bounds the no-op launches enqueued past the stop.  The caller brings
 * its iteration's bytes -- from numbers all ranks agree on where there are several -- and rounds to even where a
 * chunk has to leave the parity where it found it; opts.check_every overrides the rule, per caller. */
int run_chunk(double bytes, double floor_us, int lo, int hi) {
  double us = bytes / 4.0e6; /* 4 TB/s => bytes per microsecond */
  if (us < floor_us)
    us = floor_us;
  const int c = (int)(300.0 / us);
  return c < lo ? lo : c > hi ? hi : c;
}

/* ---- captured graphs -------------------------------------------------------------------------------------------
 * `count` iterations as plain(ctx, count) enqueues them, captured once and replayed: LSB_NGRAPH entries -- the
 * hinted whole-solve graph and the small continuation chunk, of the solve proper and of a correction -- found by
 * (count, key), replaced round-robin.  key: the one pointer of the caller's inside the launches (x), NULL where the
 * iteration touches internal buffers only. */
static hipGraphExec_t graph_get(struct graph_cache *gc, int count, const void *key, run_enqueue_fn *plain,
                                void *ctx) {
  for (int i = 0; i < LSB_NGRAPH; i++)
    if (gc->e[i].exec && gc->e[i].count == count && gc->e[i].key == key)
      return gc->e[i].exec;
  const int slot = gc->next;
  gc->next = (gc->next + 1) % LSB_NGRAPH;
  if (gc->e[slot].exec)
    LSB_CHK_HIP(hipGraphExecDestroy(gc->e[slot].exec));
  hipGraph_t g;
  LSB_CHK_HIP(hipStreamBeginCapture(g_stream, hipStreamCaptureModeThreadLocal));
  plain(ctx, count);
  LSB_CHK_HIP(hipStreamEndCapture(g_stream, &g));
  LSB_CHK_HIP(hipGraphInstantiate(&gc->e[slot].exec, g, NULL, NULL, 0));
  LSB_CHK_HIP(hipGraphDestroy(g));
  gc->e[slot].count = count, gc->e[slot].key = key;
  return gc->e[slot].exec;
}

void graph_launch(struct graph_cache *gc, int count, const void *key, run_enqueue_fn *plain, void *ctx) {
  LSB_CHK_HIP(hipGraphLaunch(graph_get(gc, count, key, plain, ctx), g_stream));
}

void graph_drop(struct graph_cache *gc) {
  for (int i = 0; i < LSB_NGRAPH; i++)
    if (gc->e[i].exec) {
      LSB_CHK_HIP(hipGraphExecDestroy(gc->e[i].exec));
      gc->e[i].exec = NULL;
    }
}

/* every cache of the solver: graphs must not outlive the buffers they were captured with */
void drop_graphs(lsb_hip_solver *sv) {
  graph_drop(&sv->graphs);
  graph_drop(&sv->rich_graphs);
  if (sv->dir)
    graph_drop(&sv->dir->graphs);
  for (int k = 0; k < 3; k++) {
    graph_drop(&sv->mr[k].blk.g), graph_drop(&sv->bk[k].blk.g), graph_drop(&sv->rm[k].blk.g);
    if (sv->dir)
      graph_drop(&sv->dir->m[k].blk.g);
  }
}

/* ---- the loop --------------------------------------------------------------------------------------------------
 * Host side of one run.  The device decides when to stop (its state: lsb_pcg_state and its kin); the host only has
 * to enqueue enough iterations and look at the state now and then:
 *   - a solver that has solved before enqueues exactly the iteration count of its previous solve in one go (the
 *     benchmark protocol repeats the same solve `trials` times, src/cholmod-impl.h:44-63) and polls once;
 *   - otherwise, and for whatever is left, chunks are enqueued one AHEAD of the poll, through the two pinned slots
 *     and ev_poll[0 / 1], so the device never waits for the host; iterations enqueued past the stop are no-op
 *     launches, and the speculative chunk behind the poll that saw the stop is drained.
 * The final state lands in slot 0; *hint becomes what this run took, in the state's own count of progress. */
static int slot_word(const struct run_loop *r, int slot, size_t off) {
  return *(const int *)((const char *)r->h_state + (size_t)slot * r->state_bytes + off);
}

static int slot_stopped(const struct run_loop *r, int slot) {
  const int w = slot_word(r, slot, r->stop_off);
  return r->stop_is_running ? !w : w != LSB_STATUS_RUNNING;
}

static void enqueue_poll(lsb_hip_solver *sv, const struct run_loop *r, int slot) {
  LSB_CHK_HIP(hipMemcpyAsync((char *)r->h_state + (size_t)slot * r->state_bytes, r->d_state, r->state_bytes,
                             hipMemcpyDeviceToHost, g_stream));
  LSB_CHK_HIP(hipEventRecord(sv->ev_poll[slot], g_stream));
}

/* asked: iterations the loop wanted on the stream; left: what the cap still lets through (< 0: no cap) */
static void put(const struct run_loop *r, long count, unsigned *asked, long *left) {
  *asked += (unsigned)count;
  if (*left >= 0)
    count = count < *left ? count : *left, *left -= count;
  if (count > 0)
    r->enqueue(r->ctx, (int)count);
}

void run_loop(lsb_hip_solver *sv, const struct run_loop *r, unsigned *hint) {
  const int before = slot_word(r, 0, r->progress_off);
  const unsigned bound = sv->o.maxit + *hint + 1u + 3u * (unsigned)r->chunk;
  unsigned asked = 0;
  long left = r->cap;
  int fin = -1; /* slot holding the final state */
  if (*hint > 0) {
    const int total = r->even ? (int)((*hint + 1) & ~1u) : (int)*hint;
    int piece = total; /* (max_piece goes with even: halved, and even again) */
    while (r->max_piece && piece > r->max_piece)
      piece = ((piece / 2) + 1) & ~1;
    for (int todo = total; todo > 0;) {
      const int c = todo >= piece ? piece : r->even ? (todo + 1) & ~1 : todo;
      put(r, c, &asked, &left);
      todo -= c;
    }
    enqueue_poll(sv, r, 0);
    wait_event(sv, sv->ev_poll[0], r->what_hinted);
    if (slot_stopped(r, 0))
      fin = 0;
  }
  if (fin < 0) {
    int cur = 0;
    put(r, r->chunk, &asked, &left);
    enqueue_poll(sv, r, 0);
    for (;;) {
      put(r, r->chunk, &asked, &left); /* one chunk ahead of the poll */
      enqueue_poll(sv, r, cur ^ 1);
      wait_event(sv, sv->ev_poll[cur], r->what_poll);
      if (slot_stopped(r, cur)) {
        fin = cur;
        break;
      }
      cur ^= 1;
      if (asked > bound) /* cannot happen: the device counts to maxit whatever the host does */
        errx(EXIT_FAILURE, "hip_cdna4: %s ran past maxit without a status", r->name);
    }
    drain_stream(sv, r->what_drain); /* the speculative chunk */
  }
  if (fin != 0)
    memcpy(r->h_state, (const char *)r->h_state + (size_t)fin * r->state_bytes, r->state_bytes);
  *hint = (unsigned)(slot_word(r, 0, r->progress_off) - before);
}

void result_from_state(struct lsb_hip_result *r, const struct lsb_pcg_state *st) {
  r->iters = (unsigned)st->iters;
  r->status = st->status;
  r->relres = st->bb > 0.0 ? sqrt(st->rr / st->bb) : 0.0;
}
