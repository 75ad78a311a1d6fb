/*
 * Host side of the direct solver (LSB_KRYLOV_DIRECT; hip_direct_drv.c applies the factor through hip_direct_t.hip):
 * a nested-dissection ordering, the symbolic count, and the explicit inverse factor W = L^-1 of P S P^T = L L^T as a
 * skyline.  Set-up, untimed, like FSAI's, AMG's and CHOLMOD's factorisation (src/cholmod-impl.h:25-26).  Plain C
 * with OpenMP; nothing here touches the device.
 *
 *   ordering   recursive bisection.  A part is cut into its connected components, in order of their lowest vertex; a
 *              component of at most ND_LEAF vertices keeps the order it has.  A larger one is searched from a
 *              pseudo-peripheral vertex (BFS, restarted from the lowest-degree vertex of the last level while the
 *              eccentricity grows, ND_TRIALS times at the most); the separator is the smallest level among those
 *              that leave at least 30 % of the component below it and 30 % above it, the lowest such level on a tie;
 *              below, above, separator is the new order, and the two sides are cut in the same way.  No such level:
 *              the component stays as it is.
 *   lower bound  the side below a level separator is connected and every separator vertex has a neighbour in it, so
 *              every separator vertex is an ancestor of every vertex below: the tree of this ordering has at least
 *              n + sum |below| |separator| entries in W.  lsb_csr_nd_bounded stops as soon as that exceeds a budget,
 *              which is how a 10 M-row grid is refused after one bisection instead of after twenty.
 *   tree       Liu's algorithm with path compression on the rows of P S P^T (lsb_csr_skyline_count: no numeric work).
 *   postorder  children in ascending order, the child with the largest subtree last: a subtree is a contiguous run of
 *              indices, parent(i) = i + 1 wherever i is a last child, and a walk to the root leaves such a run at
 *              most log2(n) times.
 *   factor     up-looking sparse Cholesky, row by row on the row subtrees, columns of L as lists.
 *   W          column j of L^-1 lives on the path j -> root: solve L w = e_j along it, column-oriented; OpenMP over
 *              columns, each of which writes its own slots.  Row k of W is the run of columns [first_k, k] (its
 *              subtree), dense: (L^-1)_kj != 0 exactly when k is an ancestor of j.
 *   tiers      for operators whose single skyline is over the budget: the tree cut by subtree size into tiers, the
 *              rows numbered tier by tier; W is kept for the diagonal blocks alone and the blocks below them are the
 *              sparse rows of L (tier_build; one tier is the single skyline, computed by the same code).
 */
#define _GNU_SOURCE
#include <math.h>
#include <omp.h>
#include <string.h>

#include "lsb_impl.h"

#define ND_LEAF 32  /* see DESIGN.md section 4 for the counts at 8 .. 128 */
#define ND_TRIALS 4
#define NONE 0xFFFFFFFFu

static int cmp_unsigned(const void *a, const void *b) {
  const unsigned x = *(const unsigned *)a, y = *(const unsigned *)b;
  return x < y ? -1 : x > y;
}

/* ---- nested dissection ---------------------------------------------------------------------------------------- */
struct nd {
  const struct csr *S;
  unsigned *perm;      /* the order being built: every part is a range of it */
  unsigned *part;      /* part[v]: id of the part v belongs to right now */
  unsigned *level;     /* level[v] of the last BFS that reached v */
  unsigned *queue;     /* BFS order, positions as in perm */
  unsigned *cnt;       /* vertices per level */
  unsigned next_id;
  unsigned long long budget, lower;
  int over;
};

/* BFS from `start` over the vertices of part `id` not yet at `stamp` in seen[]; the order goes to q[0 ..), the
 * levels into level[]; returns the count, *nlev the number of levels */
static unsigned nd_bfs(struct nd *w, unsigned start, unsigned id, unsigned *seen, unsigned stamp, unsigned *q,
                       unsigned *nlev) {
  const struct csr *S = w->S;
  unsigned head = 0, tail = 0;
  q[tail++] = start, seen[start] = stamp, w->level[start] = 0;
  while (head < tail) {
    const unsigned u = q[head++];
    for (unsigned j = S->offs[u]; j < S->offs[u + 1]; j++) {
      const unsigned v = S->cols[j] - S->base;
      if (v < S->nrows && w->part[v] == id && seen[v] != stamp)
        seen[v] = stamp, w->level[v] = w->level[u] + 1, q[tail++] = v;
    }
  }
  *nlev = w->level[q[tail - 1]] + 1;
  return tail;
}

struct nd_scratch {
  unsigned *seen, stamp;
};

static void nd_part(struct nd *w, struct nd_scratch *sc, unsigned lo, unsigned hi);

/* one connected component, all of part `id`: perm[lo .. hi) and queue[lo .. hi) hold it in BFS order from its lowest
 * vertex, level[] the nlev levels of that search */
static void nd_component(struct nd *w, struct nd_scratch *sc, unsigned lo, unsigned hi, unsigned id, unsigned nlev) {
  const struct csr *S = w->S;
  const unsigned m = hi - lo;
  if (m <= ND_LEAF || w->over)
    return;
  unsigned *q = w->queue + lo;
  /* pseudo-peripheral start: on from the lowest-degree vertex of the last level while the eccentricity grows; q and
   * level[] hold the search from the start that is kept */
  for (int trial = 1; trial < ND_TRIALS; trial++) {
    const unsigned best = nlev;
    unsigned far = q[m - 1], fdeg = NONE;
    for (unsigned k = m; k-- > 0 && w->level[q[k]] == nlev - 1;) {
      const unsigned d = S->offs[q[k] + 1] - S->offs[q[k]];
      if (d <= fdeg)
        fdeg = d, far = q[k];
    }
    nd_bfs(w, far, id, sc->seen, ++sc->stamp, q, &nlev);
    if (nlev <= best)
      break;
  }
  memset(w->cnt, 0, (size_t)nlev * sizeof(unsigned));
  for (unsigned k = 0; k < m; k++)
    w->cnt[w->level[q[k]]]++;
  const unsigned need = (unsigned)ceil(0.3 * m);
  unsigned sep = NONE, below = 0, sep_below = 0;
  for (unsigned l = 0; l < nlev; below += w->cnt[l], l++)
    if (below >= need && m - below - w->cnt[l] >= need && (sep == NONE || w->cnt[l] < w->cnt[sep]))
      sep = l, sep_below = below;
  if (sep == NONE)
    return; /* too few levels to cut: the component stays as it is */
  /* BFS order is level order: q = below | separator | above.  The new order: below, above, separator */
  const unsigned ns = w->cnt[sep], na = m - sep_below - ns;
  w->lower += (unsigned long long)sep_below * ns;
  if (w->lower > w->budget) {
    w->over = 1;
    return;
  }
  memcpy(w->perm + lo, q, (size_t)sep_below * sizeof(unsigned));
  memcpy(w->perm + lo + sep_below, q + sep_below + ns, (size_t)na * sizeof(unsigned));
  memcpy(w->perm + lo + sep_below + na, q + sep_below, (size_t)ns * sizeof(unsigned));
  for (unsigned k = lo + sep_below + na; k < hi; k++)
    w->part[w->perm[k]] = NONE; /* the separator is placed: in nobody's part any more */
  nd_part(w, sc, lo, lo + sep_below);
  nd_part(w, sc, lo + sep_below, lo + sep_below + na);
}

/* perm[lo .. hi): cut into components, each dissected */
static void nd_part(struct nd *w, struct nd_scratch *sc, unsigned lo, unsigned hi) {
  if (hi - lo <= 1 || w->over)
    return;
  const unsigned id = w->next_id++;
  for (unsigned k = lo; k < hi; k++)
    w->part[w->perm[k]] = id;
  /* components in order of their lowest vertex: the part's vertices, ascending, are the candidates */
  unsigned *q = w->queue + lo, pos = 0, nlev;
  const unsigned stamp = ++sc->stamp;
  unsigned *cand = (unsigned *)malloc((size_t)(hi - lo) * sizeof(unsigned));
  if (!cand) {
    w->over = 2;
    return;
  }
  memcpy(cand, w->perm + lo, (size_t)(hi - lo) * sizeof(unsigned));
  int sorted = 1;
  for (unsigned c = 1; c < hi - lo && sorted; c++)
    sorted = cand[c - 1] < cand[c];
  if (!sorted)
    qsort(cand, hi - lo, sizeof(unsigned), cmp_unsigned);
  unsigned ncomp = 0, *cbeg = NULL, ccap = 0; /* per component: where it begins in q, the levels of its BFS */
  for (unsigned c = 0; c < hi - lo; c++) {
    if (sc->seen[cand[c]] == stamp)
      continue;
    if (2 * ncomp + 3 > ccap) {
      ccap = ccap ? 2 * ccap : 32;
      unsigned *nb = (unsigned *)realloc(cbeg, (size_t)ccap * sizeof(unsigned));
      if (!nb) {
        free(cbeg), free(cand);
        w->over = 2;
        return;
      }
      cbeg = nb;
    }
    cbeg[2 * ncomp] = pos;
    pos += nd_bfs(w, cand[c], id, sc->seen, stamp, q + pos, &nlev);
    cbeg[2 * ncomp + 1] = nlev, ncomp++;
  }
  free(cand);
  if (ncomp)
    cbeg[2 * ncomp] = pos;
  memcpy(w->perm + lo, q, (size_t)(hi - lo) * sizeof(unsigned));
  for (unsigned c = 0; c < ncomp && !w->over; c++) {
    const unsigned c0 = lo + cbeg[2 * c], c1 = lo + cbeg[2 * c + 2];
    unsigned cid = id;
    if (ncomp > 1 && c1 - c0 > ND_LEAF) { /* a part of its own: the searches inside it must not leave it */
      cid = w->next_id++;
      for (unsigned k = c0; k < c1; k++)
        w->part[w->perm[k]] = cid;
    }
    nd_component(w, sc, c0, c1, cid, cbeg[2 * c + 1]);
  }
  free(cbeg);
}

int lsb_csr_nd_bounded(const struct csr *S, unsigned *perm, unsigned long long budget, unsigned long long *lower) {
  const unsigned n = S->nrows;
  struct nd w = {.S = S, .perm = perm, .next_id = 0, .budget = budget, .lower = n};
  struct nd_scratch sc = {NULL, 0};
  w.part = (unsigned *)malloc((size_t)(n ? n : 1) * sizeof(unsigned));
  w.level = (unsigned *)malloc((size_t)(n ? n : 1) * sizeof(unsigned));
  w.queue = (unsigned *)malloc((size_t)(n ? n : 1) * sizeof(unsigned));
  w.cnt = (unsigned *)malloc((size_t)(n ? n : 1) * sizeof(unsigned));
  sc.seen = (unsigned *)calloc(n ? n : 1, sizeof(unsigned));
  int rc = 2;
  if (w.part && w.level && w.queue && w.cnt && sc.seen) {
    for (unsigned i = 0; i < n; i++)
      perm[i] = i;
    if (w.lower > budget)
      w.over = 1;
    nd_part(&w, &sc, 0, n);
    rc = w.over == 2 ? 2 : w.over ? 3 : 0;
  }
  if (lower)
    *lower = w.lower;
  free(w.part), free(w.level), free(w.queue), free(w.cnt), free(sc.seen);
  return rc;
}

int lsb_csr_nd(const struct csr *S, unsigned *perm) { return lsb_csr_nd_bounded(S, perm, ~0ull, NULL); }

/* ---- the elimination tree ------------------------------------------------------------------------------------- */
/* parent[k] of P S P^T (NONE: a root), Liu's algorithm with path compression; inv[old] = new; anc: n unsigneds */
static void etree(const struct csr *S, const unsigned *perm, const unsigned *inv, unsigned *parent, unsigned *anc) {
  const unsigned n = S->nrows;
  for (unsigned k = 0; k < n; k++) {
    parent[k] = anc[k] = NONE;
    const unsigned row = perm[k];
    for (unsigned j = S->offs[row]; j < S->offs[row + 1]; j++) {
      const unsigned c = S->cols[j] - S->base;
      if (c >= n)
        continue;
      for (unsigned i = inv[c]; i != NONE && i < k;) {
        const unsigned next = anc[i];
        anc[i] = k;
        if (next == NONE)
          parent[i] = k;
        i = next;
      }
    }
  }
}

/* 0: perm is a permutation of 0 .. n - 1 (inv filled) */
static int invert_perm(unsigned n, const unsigned *perm, unsigned *inv) {
  for (unsigned i = 0; i < n; i++)
    inv[i] = NONE;
  for (unsigned k = 0; k < n; k++) {
    if (perm[k] >= n || inv[perm[k]] != NONE)
      return 1;
    inv[perm[k]] = k;
  }
  return 0;
}

unsigned long long lsb_csr_skyline_count(const struct csr *S, const unsigned *perm, unsigned *height) {
  const unsigned n = S->nrows;
  unsigned *inv = (unsigned *)malloc((size_t)(n ? n : 1) * sizeof(unsigned));
  unsigned *parent = (unsigned *)malloc((size_t)(n ? n : 1) * sizeof(unsigned));
  unsigned *anc = (unsigned *)malloc((size_t)(n ? n : 1) * sizeof(unsigned));
  unsigned long long total = 0;
  unsigned h = 0;
  if (inv && parent && anc && !invert_perm(n, perm, inv)) {
    etree(S, perm, inv, parent, anc);
    unsigned *depth = anc; /* parent[k] > k: the depths from the top down */
    for (unsigned k = n; k-- > 0;) {
      depth[k] = parent[k] == NONE ? 1u : depth[parent[k]] + 1u;
      total += depth[k];
      if (depth[k] > h)
        h = depth[k];
    }
  }
  if (height)
    *height = h;
  free(inv), free(parent), free(anc);
  return total;
}

/* ---- tiers ---------------------------------------------------------------------------------------------------- */
/* The thresholds of m tiers: T_i, i = 1 .. m - 1, the smallest integer with T_i^m >= n^i.  In integers, so that a
 * model in another language reproduces them: eight limbs of 32 bits hold n^5 and T^6 for every 32-bit n */
struct big {
  unsigned w[8];
};

static void big_pow(struct big *r, unsigned base, unsigned e) {
  memset(r, 0, sizeof *r);
  r->w[0] = 1;
  while (e-- > 0) {
    unsigned long long c = 0;
    for (unsigned l = 0; l < 8; l++)
      c += (unsigned long long)r->w[l] * base, r->w[l] = (unsigned)c, c >>= 32;
  }
}

static int big_ge(const struct big *a, const struct big *b) {
  for (unsigned l = 8; l-- > 0;)
    if (a->w[l] != b->w[l])
      return a->w[l] > b->w[l];
  return 1;
}

static void tier_thresholds(unsigned n, unsigned m, unsigned *T) {
  for (unsigned i = 1; i < m; i++) {
    struct big want, have;
    big_pow(&want, n, i);
    unsigned lo = 1, hi = n ? n : 1; /* n^m >= n^i */
    while (lo < hi) {
      const unsigned mid = lo + (hi - lo) / 2;
      big_pow(&have, mid, m);
      if (big_ge(&have, &want))
        hi = mid;
      else
        lo = mid + 1;
    }
    T[i - 1] = lo;
  }
}

/* tier[v] = how many of the thresholds size[v] exceeds, then the tiers nobody is in dropped; lo[t]: vertices in the
 * tiers below t (lo[ntier] = n).  A subtree is no smaller than its children's: tiers never decrease towards the root.
 * Returns ntier */
static unsigned tier_assign(unsigned n, unsigned m, const unsigned *size, unsigned *tier, unsigned *lo) {
  unsigned T[LSB_DIRECT_MAX_TIERS], cnt[LSB_DIRECT_MAX_TIERS] = {0}, map[LSB_DIRECT_MAX_TIERS] = {0}, ntier = 0;
  tier_thresholds(n, m, T);
  for (unsigned v = 0; v < n; v++) {
    unsigned t = 0;
    while (t + 1 < m && size[v] > T[t])
      t++;
    tier[v] = t, cnt[t]++;
  }
  lo[0] = 0;
  for (unsigned t = 0; t < m; t++)
    if (cnt[t])
      map[t] = ntier, lo[ntier + 1] = lo[ntier] + cnt[t], ntier++;
  if (!ntier) /* n = 0 */
    ntier = 1, lo[1] = 0;
  for (unsigned v = 0; v < n; v++)
    tier[v] = map[tier[v]];
  return ntier;
}

int lsb_csr_tiered_count(const struct csr *S, const unsigned *perm, unsigned tiers, unsigned long long *w_entries,
                         unsigned long long *coupling_entries, unsigned *height) {
  const unsigned n = S->nrows, n1 = n ? n : 1;
  unsigned long long w = 0, c = 0;
  unsigned h = 0, lo[LSB_DIRECT_MAX_TIERS + 1];
  int rc = tiers >= 1 && tiers <= LSB_DIRECT_MAX_TIERS ? 0 : 2;
  unsigned *inv = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));
  unsigned *parent = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));
  unsigned *work = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));
  unsigned *size = (unsigned *)calloc(n1, sizeof(unsigned));
  unsigned *tier = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));
  if (!rc && !(inv && parent && work && size && tier))
    rc = 3;
  if (!rc && invert_perm(n, perm, inv))
    rc = 2;
  if (!rc) {
    etree(S, perm, inv, parent, work);
    for (unsigned k = 0; k < n; k++) { /* parent > child: sizes bottom-up in index order */
      size[k] += 1;
      if (parent[k] != NONE)
        size[parent[k]] += size[k];
    }
    tier_assign(n, tiers, size, tier, lo);
    /* W_tt: a column's depth inside its tier; the height is the whole tree's.  size[] becomes the depth, work[] the
     * depth inside the tier */
    for (unsigned k = n; k-- > 0;) {
      const unsigned p = parent[k];
      size[k] = p == NONE ? 1u : size[p] + 1u;
      work[k] = p == NONE || tier[p] != tier[k] ? 1u : work[p] + 1u;
      w += work[k];
      if (size[k] > h)
        h = size[k];
    }
    /* the entries of L from the row subtrees: those that leave the row's tier are the coupling */
    unsigned *mark = work;
    for (unsigned k = 0; k < n; k++)
      mark[k] = NONE;
    for (unsigned k = 0; k < n; k++) {
      mark[k] = k;
      const unsigned row = perm[k];
      for (unsigned j = S->offs[row]; j < S->offs[row + 1]; j++) {
        const unsigned col = S->cols[j] - S->base;
        if (col >= n || inv[col] >= k)
          continue;
        for (unsigned i = inv[col]; mark[i] != k; i = parent[i])
          mark[i] = k, c += tier[i] != tier[k];
      }
    }
  }
  if (w_entries)
    *w_entries = w;
  if (coupling_entries)
    *coupling_entries = c;
  if (height)
    *height = h;
  free(inv), free(parent), free(work), free(size), free(tier);
  return rc;
}

/* ---- the factor ----------------------------------------------------------------------------------------------- */
void lsb_skyinv_free(struct lsb_skyinv *W) {
  if (!W)
    return;
  free(W->perm), free(W->first), free(W->woff), free(W->vals), free(W->parent), free(W->run_end);
  free(W);
}

void lsb_tierinv_free(struct lsb_tierinv *W) {
  if (!W)
    return;
  free(W->perm), free(W->first), free(W->woff), free(W->vals), free(W->parent), free(W->run_end);
  free(W->coffs), free(W->ccols), free(W->cvals), free(W->toffs), free(W->tcols), free(W->tvals);
  free(W);
}

/* The factor in `tiers` tiers (>= 1; one tier: the single skyline, nothing coupled).  Tier-major numbering: sorted by
 * (tier, postorder index), still an elimination order with the same fill, and the part of a subtree that lies in
 * tier t is a run of indices inside tier t's range.  L is then block lower triangular: W_tt = (L_tt)^-1 is a skyline
 * like the single one (first clipped at the tier's start, parent = n on the root of a tier's tree), and the blocks
 * below the diagonal are the rows of L itself, kept twice: C by rows, C^T by tier and lower-tier column */
static struct lsb_tierinv *tier_build(const struct csr *S, const unsigned *perm_in, unsigned tiers, int *why) {
  const unsigned n = S->nrows, n1 = n ? n : 1;
  int bad = 0;
  struct lsb_tierinv *W = lsb_calloc(struct lsb_tierinv, 1);
  unsigned *inv = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));
  unsigned *par0 = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));
  unsigned *tmp = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));
  unsigned *size = (unsigned *)calloc(n1, sizeof(unsigned));
  unsigned *head = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));
  unsigned *next = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));
  unsigned *post = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));
  unsigned *tier0 = (unsigned *)malloc((size_t)n1 * sizeof(unsigned)); /* by the index of the given ordering */
  unsigned *tier = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));  /* by the tier-major index */
  unsigned *ord = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));   /* tier-major index -> given index */
  unsigned *cc = NULL, *lrow = NULL;
  unsigned long long *lp = NULL;
  double *lval = NULL, *x = NULL;
  struct csr *B = NULL;
  if (W) {
    W->n = n;
    W->perm = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));
    W->first = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));
    W->parent = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));
    W->run_end = (unsigned *)malloc((size_t)n1 * sizeof(unsigned));
    W->woff = (unsigned long long *)calloc((size_t)n + 1, sizeof(unsigned long long));
  }
  if (!W || !inv || !par0 || !tmp || !size || !head || !next || !post || !tier0 || !tier || !ord || !W->perm ||
      !W->first || !W->parent || !W->run_end || !W->woff || invert_perm(n, perm_in, inv)) {
    bad = 3;
    goto out;
  }
  /* the tree of the given ordering, and a postorder of it: children ascending, the largest subtree last */
  etree(S, perm_in, inv, par0, tmp);
  for (unsigned k = 0; k < n; k++) { /* parent > child: sizes bottom-up in index order */
    size[k] += 1;
    if (par0[k] != NONE)
      size[par0[k]] += size[k];
  }
  for (unsigned k = 0; k < n; k++)
    head[k] = NONE;
  unsigned roots = NONE; /* lists built by descending k come out ascending */
  for (unsigned k = n; k-- > 0;) {
    unsigned *list = par0[k] == NONE ? &roots : &head[par0[k]];
    next[k] = *list, *list = k;
  }
  for (unsigned p = 0; p < n; p++) { /* the first largest child to the end of its list */
    unsigned big = NONE, prev_big = NONE, prev = NONE, last = NONE;
    for (unsigned c = head[p]; c != NONE; prev = c, c = next[c]) {
      if (big == NONE || size[c] > size[big])
        big = c, prev_big = prev;
      last = c;
    }
    if (big != NONE && big != last) {
      if (prev_big == NONE)
        head[p] = next[big];
      else
        next[prev_big] = next[big];
      next[last] = big, next[big] = NONE;
    }
  }
  {
    unsigned np = 0, top = 0, *stack = tmp;
    for (unsigned r = roots; r != NONE; r = next[r]) {
      stack[top++] = r;
      while (top) {
        const unsigned v = stack[top - 1], c = head[v];
        if (c == NONE)
          post[np++] = v, top--;
        else
          head[v] = next[c], stack[top++] = c; /* (the lists are used up) */
      }
    }
    if (np != n) {
      bad = 3;
      goto out;
    }
  }
  /* the tiers, and the postorder sorted by them (stable: inside a tier the postorder stays) */
  W->ntier = tier_assign(n, tiers, size, tier0, W->lo);
  {
    unsigned at[LSB_DIRECT_MAX_TIERS];
    memcpy(at, W->lo, sizeof at);
    for (unsigned k = 0; k < n; k++)
      ord[at[tier0[post[k]]]++] = post[k];
  }
  unsigned *full = next; /* the whole tree in the new numbering (n on a root): what the factorisation climbs */
  for (unsigned k = 0; k < n; k++)
    W->perm[k] = perm_in[ord[k]], tmp[ord[k]] = k, tier[k] = tier0[ord[k]]; /* tmp: given index -> new */
  for (unsigned k = 0; k < n; k++) {
    full[k] = par0[ord[k]] == NONE ? n : tmp[par0[ord[k]]];
    W->parent[k] = full[k] < n && tier[full[k]] == tier[k] ? full[k] : n;
  }
  unsigned *tsize = post; /* the part of k's subtree in k's own tier */
  memset(tsize, 0, (size_t)n1 * sizeof(unsigned));
  for (unsigned k = 0; k < n; k++) {
    tsize[k] += 1;
    if (W->parent[k] < n)
      tsize[W->parent[k]] += tsize[k];
    W->first[k] = k + 1 - tsize[k];
  }
  for (unsigned k = n; k-- > 0;)
    W->run_end[k] = (k + 1 < n && W->parent[k] == k + 1) ? W->run_end[k + 1] : k;
  for (unsigned k = 0; k < n; k++)
    W->woff[k + 1] = W->woff[k] + (k - W->first[k] + 1);
  if (W->woff[n] > LSB_DIRECT_MAX_ENTRIES) {
    bad = 2;
    goto out;
  }
  /* P S P^T with sorted rows; column counts of L from the row subtrees */
  B = lsb_csr_permute_sym(S, W->perm);
  cc = (unsigned *)calloc(n1, sizeof(unsigned));
  lp = (unsigned long long *)calloc((size_t)n + 1, sizeof(unsigned long long));
  x = (double *)calloc(n1, sizeof(double));
  if (!B || !cc || !lp || !x) {
    bad = 3;
    goto out;
  }
  unsigned *mark = inv, *pat = head;
  unsigned long long coupling = 0;
  for (unsigned k = 0; k < n; k++)
    mark[k] = NONE;
  for (unsigned k = 0; k < n; k++) {
    mark[k] = k;
    for (unsigned j = B->offs[k]; j < B->offs[k + 1] && B->cols[j] < k; j++)
      for (unsigned i = B->cols[j]; mark[i] != k; i = full[i])
        mark[i] = k, cc[i]++, coupling += tier[i] != tier[k];
  }
  if (W->woff[n] + 3 * coupling > LSB_DIRECT_MAX_ENTRIES) { /* C and C^T: 12 B an entry each */
    bad = 2;
    goto out;
  }
  for (unsigned k = 0; k < n; k++)
    lp[k + 1] = lp[k] + cc[k];
  lrow = (unsigned *)malloc((size_t)(lp[n] ? lp[n] : 1) * sizeof(unsigned));
  lval = (double *)malloc((size_t)(lp[n] ? lp[n] : 1) * sizeof(double));
  W->vals = (double *)malloc((size_t)(W->woff[n] ? W->woff[n] : 1) * sizeof(double));
  double *diag = (double *)malloc((size_t)n1 * sizeof(double));
  if (!lrow || !lval || !W->vals || !diag) {
    free(diag);
    bad = 3;
    goto out;
  }
  /* up-looking: row k of L solves L[0:k, 0:k] l = B[0:k, k] on the row subtree, ascending */
  memset(cc, 0, (size_t)n1 * sizeof(unsigned)); /* entries of column j filled so far */
  for (unsigned k = 0; k < n; k++)
    mark[k] = NONE;
  for (unsigned k = 0; k < n && !bad; k++) {
    unsigned np = 0;
    double d = 0.0;
    mark[k] = k;
    for (unsigned j = B->offs[k]; j < B->offs[k + 1]; j++) {
      const unsigned c = B->cols[j];
      if (c > k)
        break;
      if (c == k) {
        d = B->vals[j];
        continue;
      }
      x[c] = B->vals[j];
      for (unsigned i = c; mark[i] != k; i = full[i])
        mark[i] = k, pat[np++] = i;
    }
    qsort(pat, np, sizeof(unsigned), cmp_unsigned);
    for (unsigned t = 0; t < np; t++) {
      const unsigned j = pat[t];
      const double lkj = x[j] / diag[j];
      x[j] = 0.0;
      for (unsigned long long p = lp[j]; p < lp[j] + cc[j]; p++)
        x[lrow[p]] -= lval[p] * lkj;
      d -= lkj * lkj;
      lrow[lp[j] + cc[j]] = k, lval[lp[j] + cc[j]] = lkj, cc[j]++;
    }
    if (!(d > 0.0) || !isfinite(d))
      bad = 1;
    diag[k] = sqrt(d);
  }
  if (!bad) {
    /* column j of W_tt = (L_tt)^-1 on the path j -> the root of its tier's tree: w_j = 1 / l_jj; ascending m on the
     * path, w_m final, then w_i -= l_im w_m for the rows i of column m in this tier (ancestors of m: on the path; the
     * rows of a column ascend, so they come first in its list), and w_i /= l_ii when its turn comes */
    int oom = 0;
#pragma omp parallel
    {
      double *w = (double *)calloc(n1, sizeof(double));
      if (!w) {
#pragma omp atomic write
        oom = 1;
      }
#pragma omp for schedule(dynamic, 64)
      for (long long jj = 0; jj < (long long)n; jj++) {
        if (!w)
          continue;
        const unsigned j = (unsigned)jj, hi = W->lo[tier[j] + 1];
        w[j] = 1.0;
        for (unsigned m = j; m < n; m = W->parent[m]) {
          const double wm = w[m] / diag[m];
          w[m] = 0.0;
          W->vals[W->woff[m] + (j - W->first[m])] = wm;
          for (unsigned long long p = lp[m]; p < lp[m + 1] && lrow[p] < hi; p++)
            w[lrow[p]] -= lval[p] * wm;
        }
      }
      free(w);
    }
    if (oom)
      bad = 3;
  }
  free(diag);
  if (!bad) {
    /* C: the rows of tiers >= 1, row i at coffs[i - lo[1]], columns ascending (filled column by column).  C^T: for
     * t = 1 .. ntier - 1 the columns j < lo[t] with their rows in tier t, lo[t] + 1 offsets each, one after another
     * (tier t's begin at the sum of lo[s] + 1 over 1 <= s < t); cc[j] walks column j's list, whose rows ascend through the tiers */
    const unsigned lo1 = W->lo[1 < W->ntier ? 1 : W->ntier], nc = n - lo1;
    size_t nt = 1;
    for (unsigned t = 1; t < W->ntier; t++)
      nt += (size_t)W->lo[t] + 1;
    W->coffs = (unsigned *)calloc((size_t)nc + 1, sizeof(unsigned));
    W->ccols = (unsigned *)malloc((size_t)(coupling ? coupling : 1) * sizeof(unsigned));
    W->cvals = (double *)malloc((size_t)(coupling ? coupling : 1) * sizeof(double));
    W->toffs = (unsigned *)calloc(nt, sizeof(unsigned));
    W->tcols = (unsigned *)malloc((size_t)(coupling ? coupling : 1) * sizeof(unsigned));
    W->tvals = (double *)malloc((size_t)(coupling ? coupling : 1) * sizeof(double));
    if (!W->coffs || !W->ccols || !W->cvals || !W->toffs || !W->tcols || !W->tvals) {
      bad = 3;
      goto out;
    }
    for (unsigned j = 0; j < n; j++) {
      unsigned long long p = lp[j];
      while (p < lp[j + 1] && lrow[p] < W->lo[tier[j] + 1])
        p++;
      cc[j] = (unsigned)(p - lp[j]); /* where column j leaves its own tier */
      for (; p < lp[j + 1]; p++)
        W->coffs[lrow[p] - lo1 + 1]++;
    }
    for (unsigned i = 0; i < nc; i++)
      W->coffs[i + 1] += W->coffs[i];
    unsigned *fill = mark;
    memcpy(fill, W->coffs, (size_t)nc * sizeof(unsigned));
    for (unsigned j = 0; j < n; j++)
      for (unsigned long long p = lp[j] + cc[j]; p < lp[j + 1]; p++) {
        const unsigned e = fill[lrow[p] - lo1]++;
        W->ccols[e] = j, W->cvals[e] = lval[p];
      }
    unsigned e = 0;
    size_t at = 0;
    for (unsigned t = 1; t < W->ntier; t++) {
      for (unsigned j = 0; j < W->lo[t]; j++) {
        W->toffs[at++] = e;
        for (; lp[j] + cc[j] < lp[j + 1] && lrow[lp[j] + cc[j]] < W->lo[t + 1]; cc[j]++)
          W->tcols[e] = lrow[lp[j] + cc[j]], W->tvals[e] = lval[lp[j] + cc[j]], e++;
      }
      W->toffs[at++] = e;
    }
  }
out:
  free(inv), free(par0), free(tmp), free(size), free(head), free(next), free(post), free(tier0), free(tier), free(ord);
  free(cc), free(lp), free(lrow), free(lval), free(x);
  lsb_csr_free(B);
  if (why)
    *why = bad;
  if (bad) {
    lsb_tierinv_free(W);
    return NULL;
  }
  return W;
}

struct lsb_skyinv *lsb_csr_skyline_inverse(const struct csr *S, const unsigned *perm_in, int *why) {
  struct lsb_tierinv *T = tier_build(S, perm_in, 1, why);
  struct lsb_skyinv *W = T ? lsb_calloc(struct lsb_skyinv, 1) : NULL;
  if (!W) {
    if (T && why)
      *why = 3;
    lsb_tierinv_free(T);
    return NULL;
  }
  W->n = T->n, W->perm = T->perm, W->first = T->first, W->woff = T->woff, W->vals = T->vals;
  W->parent = T->parent, W->run_end = T->run_end;
  T->perm = T->first = T->parent = T->run_end = NULL, T->woff = NULL, T->vals = NULL;
  lsb_tierinv_free(T);
  return W;
}

struct lsb_tierinv *lsb_csr_tiered_inverse(const struct csr *S, const unsigned *perm_in, unsigned tiers, int *why) {
  if (tiers > LSB_DIRECT_MAX_TIERS) {
    if (why)
      *why = 3;
    return NULL;
  }
  if (tiers == 0) { /* the fewest tiers that fit, by the symbolic count alone */
    for (tiers = 1; tiers < LSB_DIRECT_MAX_TIERS; tiers++) {
      unsigned long long w = 0, c = 0;
      const int rc = lsb_csr_tiered_count(S, perm_in, tiers, &w, &c, NULL);
      if (rc) {
        if (why)
          *why = 3;
        return NULL;
      }
      if (w + 3 * c <= LSB_DIRECT_MAX_ENTRIES)
        break;
    }
  }
  return tier_build(S, perm_in, tiers, why);
}
