/*
 * openr_spf.h — the C ABI of the MI355X SPF engine (the ONLY entry point to
 * the HIP kernels).  Plain pointers and sizes, no C++ or torch types.
 *
 * What it replaces.  Open/R has no FFI for this path: the boundary is the C++
 * class API of LinkState / SpfSolver.  Every function below replaces the inner
 * arithmetic of one reference member function; the re-implemented LinkState
 * (openr_amd/csrc/host/LinkState.cpp) is the only caller:
 *
 *   spf_graph_create / spf_graph_destroy
 *       replaces the adjacency graph the reference walks in place:
 *       LinkState::linkMap_ / nodeOverloads_   (openr/decision/LinkState.h:457-463)
 *       and Link::isUp / getMetricFromNode     (openr/decision/LinkState.cpp:195-236)
 *   spf_graph_set_transit
 *       replaces LinkState::isNodeOverloaded as read by runSpf
 *                                               (openr/decision/LinkState.cpp:829-836)
 *   spf_query_create / spf_query_run / spf_query_sync
 *       replaces LinkState::runSpf(src, useLinkMetric, linksToIgnore)
 *                                               (openr/decision/LinkState.cpp:806-880)
 *       batched over many sources (getSpfResult memo fill, LFA neighbours,
 *       all-sources views, KSP2 second passes, what-if link failures).
 *   spf_query_dist / spf_query_nexthops / spf_query_order
 *       replace the reads of NodeSpfResult::metric / nextHops / pathLinks
 *       order                                   (openr/decision/LinkState.h:203-257)
 *
 * Conventions
 *   - Status: 0 = OK, negative = error (SPF_E_*).  No exceptions cross the ABI.
 *   - Ownership: every device buffer is owned by the handle that allocated it.
 *     Host buffers passed in are read during the call only; host output
 *     buffers are caller-allocated and filled synchronously.
 *   - Lifetime: a handle must outlive every handle created over it — queries
 *     over a graph, route tables over a query, cluster graphs and tables over
 *     a cluster, tables over a cluster graph.  Destroying a handle while
 *     dependants are alive is refused: spf_graph_destroy, spf_query_destroy,
 *     spf_cgraph_destroy and spf_cluster_destroy then return SPF_E_INVALID
 *     and free nothing (the handle stays valid; destroy the dependants, then
 *     call again).  This mirrors the reference's contract that SpfResult
 *     references stay valid until the next topology change
 *     (openr/decision/LinkState.h:269-275).  Destroying NULL is a no-op.
 *   - Threading: a graph and its queries are used from one host thread.  All
 *     work of a graph is enqueued on one HIP stream (spf_graph_set_stream).
 *   - Node ids are 0..V-1 and MUST equal the lexicographic rank of the node
 *     name (the reference breaks Dijkstra ties by name, LinkState.h:488-498).
 *   - There is no CPU fallback: without a usable gfx950 device every call that
 *     needs one returns SPF_E_DEVICE.
 */
#ifndef OPENR_SPF_H
#define OPENR_SPF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPF_OK 0
#define SPF_E_INVALID (-1)     /* bad argument / shape */
#define SPF_E_NOMEM (-2)       /* device or host allocation failed */
#define SPF_E_DEVICE (-3)      /* HIP runtime error / no device */
#define SPF_E_UNSUPPORTED (-4) /* shape outside what the kernels handle */

#define SPF_UNREACHABLE UINT64_MAX

/* query flags */
#define SPF_F_UNIT_METRIC 0x1u /* useLinkMetric == false: every hop costs 1 */
#define SPF_F_NEXTHOPS 0x2u    /* compute ECMP next-hop sets */
#define SPF_F_ORDER 0x4u       /* keep the settle order (pathLinks ordering) */

/* Directed CSR of the UP links of one area (Link::isUp, LinkState.cpp:233).
 * Every undirected link contributes two half-edges e (u->v) and rev[e]
 * (v->u) that share link_id.  metric[e] is the metric advertised by the row
 * node u (Link::getMetricFromNode(u)), as the reference's uint64
 * LinkStateMetric (an i32 adjacency metric sign-extended, LinkState.h:22). */
typedef struct spf_graph_desc {
  uint32_t num_nodes;             /* V */
  uint32_t num_edges;             /* E (directed half-edges) */
  const uint32_t* row_ptr;        /* [V+1] */
  const uint32_t* col;            /* [E] other endpoint */
  const uint64_t* metric;         /* [E] metric advertised by the row node */
  const uint32_t* link_id;        /* [E] undirected link id (< num_links) */
  const uint32_t* rev;            /* [E] index of the reverse half-edge */
  const uint8_t* node_overloaded; /* [V] 1 = no transit (isNodeOverloaded) */
  uint32_t num_links;             /* number of distinct link ids */
  int device;                     /* HIP device ordinal */
} spf_graph_desc;

typedef struct spf_graph spf_graph;
typedef struct spf_query spf_query;

/* One batch of single-source SPF runs.  Query i runs from sources[i]; when
 * ignore_offsets is non-NULL query i skips the links
 * ignore_links[ignore_offsets[i] .. ignore_offsets[i+1]) (sorted ascending,
 * the linksToIgnore set of LinkState::runSpf / getKthPaths k>=2). */
typedef struct spf_query_desc {
  uint32_t num_queries;
  const uint32_t* sources;        /* [num_queries] */
  const uint32_t* ignore_offsets; /* [num_queries+1] or NULL */
  const uint32_t* ignore_links;   /* sorted per query, or NULL */
  uint32_t flags;                 /* SPF_F_* */
} spf_query_desc;

/* ---- device ---- */
int spf_device_count(void);
const char* spf_error_string(int status);
const char* spf_last_error_detail(void); /* thread-local text of last error */

/* ---- device memory (tables a host driver owns, e.g. AllSourcesTable) ---- */
#define SPF_COPY_D2H 0
#define SPF_COPY_H2D 1
#define SPF_COPY_D2D 2
int spf_device_alloc(int device, size_t bytes, void** out);
int spf_device_free(int device, void* p);
/* synchronous copy on `device` (SPF_COPY_*) */
int spf_device_memcpy(int device, void* dst, const void* src, size_t bytes, int kind);

/* ---- graph ---- */
int spf_graph_create(const spf_graph_desc* desc, spf_graph** out);
int spf_graph_destroy(spf_graph* g);
/* Replace the per-node transit bits (overload/drain) in place: node
 * overload toggles are the common churn (DecisionBenchmark.cpp:600-626). */
int spf_graph_set_transit(spf_graph* g, const uint8_t* node_overloaded);
/* Patch metrics of existing half-edges in place (metric churn, a7 deltas).
 * A few edges (n * 64 <= E): only their device words are rewritten. */
int spf_graph_patch_metrics(
    spf_graph* g, uint32_t n, const uint32_t* edge_idx, const uint64_t* metric);
/* Take half-edges down (up[i] = 0) or bring them back up (1) with the given
 * metrics, in place: link removal / re-addition (LinkState.cpp:421-434
 * removeLink / addLink; the reference drops its whole memo, :712-715) without
 * a new device graph.  A down half-edge stays at its CSR position as a
 * self-loop of its tail (never relaxed, never tight); the distinct-neighbour
 * lists (spf_graph_nbrs, the next-hop mask bits) are rebuilt over the up
 * half-edges, so next-hop queries stay exact.  A graph changed this way
 * refuses SPF_F_ORDER (SPF_E_UNSUPPORTED) — rebuild it for settle orders.
 * SPF_E_UNSUPPORTED too for 64-bit graphs, metric 0, or metrics the packed
 * edge words cannot hold. */
int spf_graph_set_edges(
    spf_graph* g, uint32_t n, const uint32_t* edge_idx, const uint8_t* up,
    const uint64_t* metric);
/* Which half-edges are up: up[i] = 0 iff half-edge first + i was taken down by
 * spf_graph_set_edges and not brought back (all ones on a graph that call never
 * changed, and after spf_graph_update).  Host only, no device work.
 * SPF_E_INVALID when [first, first + n) is no range of the graph's half-edges. */
int spf_graph_edge_up(const spf_graph* g, uint32_t first, uint32_t n, uint8_t* up);
/* Rebuild the graph in place from a new CSR of the same node set (a link
 * added or removed: LinkState::updateAdjacencyDatabase's structural changes,
 * LinkState.cpp:421-434 / :564-717) without a new handle: same device and
 * stream, device buffers reused where they fit.  SPF_E_INVALID while a query
 * of the graph is alive or when num_nodes differs.  On any other failure the
 * graph is left unusable: destroy it. */
int spf_graph_update(spf_graph* g, const spf_graph_desc* desc);
/* Work of this graph is enqueued on `stream` (a hipStream_t, NULL = the
 * graph's own stream). */
int spf_graph_set_stream(spf_graph* g, void* stream);
void* spf_graph_get_stream(spf_graph* g);
/* 1 if metric runs on this graph need 64-bit rows and a settle order: metric
 * 0 or sums that may pass 32 bits (the wide plan), or metrics that wrap
 * (negative i32, the literal DijkstraQ replay). */
int spf_graph_needs_exact(const spf_graph* g);
/* Number of distinct neighbours of `node` = bits in its next-hop masks. */
int spf_graph_num_nbrs(const spf_graph* g, uint32_t node);
/* The distinct neighbours of `node`, ascending by id; bit b of a next-hop
 * mask of a query from `node` stands for out[b]. */
int spf_graph_nbrs(const spf_graph* g, uint32_t node, uint32_t* out);

/* ---- queries ---- */
int spf_query_create(spf_graph* g, const spf_query_desc* desc, spf_query** out);
int spf_query_destroy(spf_query* q);
/* Enqueue the batch on the graph stream (asynchronous).
 *
 * A query may be run again after the graph changed under it in place
 * (spf_graph_set_transit, spf_graph_patch_metrics, spf_graph_set_edges).  Its
 * plan was fixed by spf_query_create, so the run does one of two things:
 *   - it computes exactly what a query created now over the same sources,
 *     flags and ignore lists would compute (distances bit for bit; next-hop
 *     sets equal, mask bits by the graph's current spf_graph_nbrs); or
 *   - it returns SPF_E_INVALID with a detail that begins "stale query:" and
 *     names the fact that moved, records and launches nothing, and leaves the
 *     last run's results readable.  Destroy the query and create a new one.
 * It never returns wrong rows.  The sub-queries a query owns (what-if
 * baselines and first-hop rows, the zero-metric plan's wide sources) are
 * covered by it.
 *
 * What a live query survives: any transit change that leaves
 * spf_graph_needs_exact as it was; any metric patch under SPF_F_UNIT_METRIC;
 * metric patches that keep the graph's class (weighted stays 32-bit and, where
 * the plan reads packed edge words or LDS rows, packable and at most 4,094;
 * uniform stays uniform at any value; the metric-0 half-edges stay the same
 * set and the zero-metric plan keeps one nonzero value); links down and up
 * after which every source keeps its next-hop mask width (1, 2, 4 or 8k
 * bytes per node) and every up neighbour has a row in a batch whose next hops
 * come from rows.
 * What it does not: a change of spf_graph_needs_exact; a uniform metric that
 * ends under any query created while it held (whatever its plan, unless
 * SPF_F_UNIT_METRIC); metric 0 or a wrapping metric introduced or
 * removed; one half of a link down alone; a mask width class crossed; a
 * neighbour that came up without a row in the batch; SPF_F_ORDER after
 * spf_graph_set_edges. */
int spf_query_run(spf_query* q);
/* 1 if spf_query_run would refuse q as stale, else 0 (also for NULL).  Host
 * only: one integer compare while the graph is unchanged since the last
 * call; per-source work only after spf_graph_set_edges. */
int spf_query_stale(const spf_query* q);
/* Wait for the last run to finish. */
int spf_query_sync(spf_query* q);
/* Device time of the last run's kernels (HIP events), milliseconds. */
int spf_query_elapsed_ms(spf_query* q, float* ms);
/* Device time of the last run split per stage: the distance kernel (plus
 * its small setup memset) and the next-hop kernel of two-stage plans
 * (nh_ms = 0 for single-kernel plans). */
int spf_query_stage_ms(spf_query* q, float* dist_ms, float* nh_ms);
/* The same split for each of the last min(n, runs, 64) runs, oldest first
 * (lets a caller time a loop of asynchronous runs per kernel). */
int spf_query_stage_history(
    spf_query* q, uint32_t n, float* dist_ms, float* nh_ms, uint32_t* got);
/* What-if screen of the last run (batches with ignore lists): *screened =
 * queries whose ignored links were all off the baseline's shortest-path DAG
 * (rows copied from the baseline, no SSSP), *has_screen = 0 when the query
 * has no screen (every query ran its own SSSP).  Synchronises the query. */
int spf_query_screened(spf_query* q, uint32_t* screened, uint32_t* has_screen);
/* Name of the plan the last run used ("lds", "dstep", "msbfs+levels", "wide",
 * "exact", ...). */
const char* spf_query_kernel_name(const spf_query* q);
/* The HIP kernels the last run launched (its sub-queries' included, and the
 * trace calls' since that run: spf_query_trace_paths), sorted
 * and comma-separated, as rocprofv3 names them without template arguments;
 * writes at most cap - 1 bytes and a NUL into buf (may be NULL) and returns
 * the full length, or a negative status.  Lets a measurement check that a
 * profile was taken of the same plan. */
int spf_query_kernels(const spf_query* q, char* buf, size_t cap);

/* Distances of query i, one per node; SPF_UNREACHABLE = not reached. */
int spf_query_dist(spf_query* q, uint32_t i, uint64_t* out /*[V]*/);
/* Words per next-hop mask of query i (ceil(nbrs(src)/64), at least 1). */
int spf_query_nh_words(const spf_query* q, uint32_t i);
/* Next-hop masks of query i: out[v*W + w], W = spf_query_nh_words (host
 * layout: u64 words, whatever the device layout). */
int spf_query_nexthops(spf_query* q, uint32_t i, uint64_t* out /*[V*W]*/);
/* Device layout of the next-hop masks (spf_query_device_rows): query i's row
 * holds spf_query_nh_bytes(q, i) bytes per node, node-major, starting
 * spf_query_nh_offset bytes into the block.  Bytes per node = 1, 2 or 4 for
 * a source with at most 8, 16 or 32 distinct neighbours (bit j of that
 * little-endian integer = the j-th neighbour, spf_graph_nbrs order), else
 * 8 * nh_words (u64 words).  Rows start 32-byte aligned. */
#define SPF_NH_BYTES(nbrs) \
  ((nbrs) <= 8u ? 1u : (nbrs) <= 16u ? 2u : (nbrs) <= 32u ? 4u : 8u * (((nbrs) + 63u) / 64u))
int spf_query_nh_bytes(const spf_query* q, uint32_t i);
int spf_query_nh_offset(const spf_query* q, uint32_t i, uint64_t* byte_off);
/* Settle rank of every node for query i (SPF_F_ORDER): the order in which the
 * reference's DijkstraQ extracts nodes; UINT32_MAX = not reached. */
int spf_query_order(spf_query* q, uint32_t i, uint32_t* out /*[V]*/);
/* Settle keys of query i (SPF_F_ORDER on a graph that needs 64-bit rows and
 * whose metrics do not wrap, i.e. the wide plan): node u settles before node v
 * iff (dist[u], key[u]) < (dist[v], key[v]) lexicographically, so a caller
 * compares instead of sorting; SPF_UNREACHABLE = not reached.
 * SPF_E_UNSUPPORTED for the literal-replay plan (use spf_query_order). */
int spf_query_order_keys(spf_query* q, uint32_t i, uint64_t* out /*[V]*/);
/* Device pointers of the result rows (for RCCL gathers): dist rows are
 * uint32 (fast kernels) or uint64 (exact kernel), spf_query_row_stride
 * elements apart (V entries used per row).  Next-hop rows are packed in the
 * byte layout of spf_query_nh_bytes: query i starts at byte
 * sum_{j<i} roundup32(V * nh_bytes(j)); *nh_total_words = the block's size
 * in 8-byte words. */
int spf_query_device_rows(
    spf_query* q, void** dist_rows, uint32_t* dist_elem_bytes,
    void** nh_rows, uint64_t* nh_total_words);
/* Copy distance rows [first, first+count) as uint32 (V entries each,
 * SPF_UNREACHABLE -> 0xFFFFFFFF) into dst, dst_pitch bytes apart: device
 * memory (asynchronous, on the graph stream — e.g. a slice of a tensor an
 * RCCL all-gather then exchanges) or host memory (synchronous).  The
 * all-sources counterpart of reading NodeSpfResult::metric() per node
 * (LinkState.h:203-257).  SPF_E_UNSUPPORTED for 64-bit (exact) rows. */
int spf_query_fetch_rows(
    spf_query* q, uint32_t first, uint32_t count, void* dst, size_t dst_pitch,
    int dst_on_device);
/* Elements between consecutive distance rows (>= V). */
uint32_t spf_query_row_stride(const spf_query* q);
/* The batch's 8-bit level rows into a level slot of a SPF_T_GATHER_LEVELS
 * table (below), after a run, asynchronously on the graph stream: on the
 * MS-BFS plan (uniform metric or SPF_F_UNIT_METRIC, many sources) query i's
 * row holds one byte per node, distance = level * scale, 255 = not reached,
 * exact while no level of the run reached 255.  Rows [0, num_queries) are
 * copied to dst_dev, dst_pitch (>= V) bytes apart, and a small kernel writes
 * the 16-byte trailer at trailer_dev: four uint32 words, [0] flags (bit 0
 * "deep": a level >= 255 occurred in THIS run; bit 1: the query has no level
 * rows -- another plan, the zero-metric variant plan, 64-bit rows, a what-if
 * batch behind a screen -- and nothing but the trailer is written), [1]
 * scale, [2] the row count, [3] 0.  Both pointers are device memory of the
 * graph's device. */
int spf_query_pack_levels(spf_query* q, void* dst_dev, size_t dst_pitch, void* trailer_dev);
/* Copy the next-hop masks of queries [first, first+count) to host memory in
 * one transfer, back to back: query i occupies V * nh_words(i) words.  The
 * bulk counterpart of spf_query_nexthops for batches whose every row the
 * caller materialises (NodeSpfResult::nextHops, LinkState.h:203-257). */
int spf_query_fetch_nexthops(
    spf_query* q, uint32_t first, uint32_t count, uint64_t* dst);
/* Both of the above into host memory with ONE synchronisation: the uint32
 * distance rows of queries [first, first+count) into rows (row_pitch bytes
 * apart; NULL skips them) and their next-hop masks into masks (the layout of
 * spf_query_fetch_nexthops; NULL skips them).  Small batches (a RouteDb
 * build's few sources: the node and its LFA neighbours, LinkState.cpp:
 * 1220-1260's per-source getSpfResult) go through a pinned staging buffer,
 * so the two transfers cost one round trip; larger ones take the two calls
 * above.  Same errors as those. */
int spf_query_fetch_host(
    spf_query* q, uint32_t first, uint32_t count, uint32_t* rows, size_t row_pitch,
    uint64_t* masks);
/* getKthPaths' trace loop on the device (LinkState.cpp:776-786 over
 * traceOnePath, :398-419): for queries [first, first+count), repeated
 * traceOnePath from the query's source to dests[i] over the query's own
 * distance row and ignore list, sharing one visited-link set, until a trace
 * fails — the KSP2 second passes of a RouteDb build (SpfSolver
 * selectKsp2 -> getKthPaths(src, dst, 2)) without their rows leaving HBM.
 * Same paths in the same order as the reference (pathLinks order: tail
 * settle rank, then linksFromNode order).  Per query i (host arrays):
 * path_count[i] paths and link_count[i] links in them, or path_count[i] =
 * SPF_TRACE_OVERFLOW when the visited set, the recursion stack or the
 * 1,024-link output of the query was exceeded (trace that query on the
 * host).  The paths stay on the device until spf_query_trace_fetch.
 * SPF_E_UNSUPPORTED for 64-bit (exact) rows. */
#define SPF_TRACE_OVERFLOW 0xFFFFFFFFu
int spf_query_trace_paths(
    spf_query* q, uint32_t first, uint32_t count, const uint32_t* dests, uint32_t* path_count,
    uint32_t* link_count);
/* The last trace's paths, packed in query order (overflowed queries
 * skipped): links[] holds Σ link_count link ids, each path src -> dst;
 * ends[] holds Σ path_count end offsets, each relative to its query's first
 * link. */
int spf_query_trace_fetch(spf_query* q, uint32_t* links, uint32_t* ends);
/* selectKsp2's walk over the traced paths on the device (Decision.cpp:970-
 * 1011 without the prepend label): per path the sum of the directional link
 * metrics from the query's source (always the link metric, also for a
 * SPF_F_UNIT_METRIC query), and the node labels of its hops after the first
 * in PUSH-stack order -- the destination's label first, the second node's
 * last; links - 1 of them.  node_labels: [V] host array.  Call after
 * spf_query_trace_paths (before or after spf_query_trace_fetch), valid until
 * the next trace or run; SPF_E_INVALID when there is no trace since the last
 * run, SPF_E_UNSUPPORTED for 64-bit rows and for a graph patched by
 * spf_graph_set_edges.  A path whose link id is >= num_links, whose link
 * lacks a half-edge or is not incident to the node the walk is at gets
 * cost SPF_EXPAND_INVALID and zero labels (never a device-traced path).
 * spf_query_trace_expand_fetch packs like spf_query_trace_fetch (overflowed
 * queries skipped): cost[Σ path_count], labels[Σ (link_count - path_count)],
 * the labels of path p of a query at (its first link) - p from the query's
 * label base. */
#define SPF_EXPAND_INVALID UINT64_MAX
int spf_query_trace_expand(spf_query* q, const int32_t* node_labels);
int spf_query_trace_expand_fetch(spf_query* q, uint64_t* cost, int32_t* labels);
/* The same kernel over caller-supplied paths of one graph (k = 1 paths
 * traced on the host): path i starts at node sources[i] and takes
 * links[off[i] .. off[i + 1]).  cost[num_paths]; labels[Σ max(len_i - 1, 0)]
 * in path order (= off[n] - n entries, path i at off[i] - i, while no path
 * is empty).  An empty path is invalid (SPF_EXPAND_INVALID, no labels).
 * SPF_E_INVALID for sources[i] >= V or descending offsets.  Metrics are
 * read at 64 bits, so every graph is supported but one patched by
 * spf_graph_set_edges (SPF_E_UNSUPPORTED). */
int spf_graph_expand_paths(
    spf_graph* g, uint32_t num_paths, const uint32_t* sources, const uint32_t* off,
    const uint32_t* links, const int32_t* node_labels, uint64_t* cost, int32_t* labels);

/* ---- incremental all-sources tables ----
 * The reference drops every memoized SpfResult on any topology change
 * (LinkState.cpp:510-511, 712-715, 728-729, driven by the LinkStateChange
 * of updateAdjacencyDatabase :564-717) and recomputes each source on
 * demand.  Here a resident table of distance rows is repaired instead: the
 * change between two graphs over the same node ids is listed as directed
 * edge deltas, a screen kernel finds the sources whose shortest-path DAG a
 * delta can touch, and only those are recomputed and scattered back. */

#define SPF_DELTA_REMOVED 1u /* usable before the change, not after */
#define SPF_DELTA_ADDED 2u   /* usable after the change, not before */
#define SPF_SCOPE_ALL 0u       /* the tail relaxes it for every source */
#define SPF_SCOPE_TAIL_ONLY 1u /* only for source == tail (tail overloaded) */
#define SPF_SCOPE_NOT_TAIL 2u  /* every source but the tail (transit flip) */

typedef struct spf_edge_delta {
  uint32_t tail, head; /* node ids shared by both graphs */
  uint64_t metric;     /* metric in the graph where the edge is usable */
  uint32_t kind;       /* SPF_DELTA_* */
  uint32_t scope;      /* SPF_SCOPE_* */
} spf_edge_delta;

/* Host-only (no device): the directed edge deltas turning `before` into
 * `after`, which must have the same num_nodes (ids = name ranks).  Per tail
 * node: half-edges (head, metric) only in `before` are REMOVED, only in
 * `after` ADDED (multiset difference, so parallel links count), and when the
 * tail's overload bit flipped its unchanged half-edges are REMOVED / ADDED
 * with SPF_SCOPE_NOT_TAIL (an overloaded node still expands as the source,
 * LinkState.cpp:829-836).  Writes min(n, cap) deltas, *n_out = n. */
int spf_graph_diff(
    const spf_graph_desc* before, const spf_graph_desc* after,
    spf_edge_delta* out, uint32_t cap, uint32_t* n_out);
/* Screen the uint32 distance rows of `num_rows` sources against the deltas
 * (kernel spf_table_screen_kernel on the graph stream): row i is affected
 * iff some delta (u, v, w) in scope of sources[i] with d[u] reached has
 * d[u] + w == d[v] (REMOVED: a tight edge of the DAG disappears) or
 * d[u] + w <= d[v] (ADDED: a new tight or shorter edge).  Unaffected rows
 * keep their distances and next-hop sets exactly (both are defined by the
 * tight usable edges alone).  `rows` is device memory, `pitch` elements
 * apart; `sources` and `affected` (one byte per row) are host memory. */
int spf_table_screen(
    spf_graph* g, const uint32_t* rows, size_t pitch, uint32_t num_rows,
    const uint32_t* sources, const spf_edge_delta* deltas, uint32_t n_deltas,
    uint8_t* affected);
/* Repair rows in place instead of recomputing them: rows[row_idx[i]]
 * (device table, pitch elements apart) hold source sources[i]'s distances
 * on the graph before a change, `g` is the graph after it and `deltas` =
 * spf_graph_diff(before, after).  Per row (spf_dstep_kernel, seeded mode):
 * nodes whose every shortest path may have used a REMOVED edge are found
 * (tight-edge closure from the removed tight edges) and those no longer
 * supported by a surviving tight path are reset to unreached; every value is
 * then an upper bound, and label-correcting delta-stepping from the reset
 * boundary and the tails of the ADDED edges lowers the row to g's distances
 * exactly, touching only the region that changed.  SPF_E_UNSUPPORTED when
 * the bucket image does not fit LDS or g needs the exact kernel (then
 * recompute the rows).  Synchronous. */
int spf_table_repair(
    spf_graph* g, uint32_t* rows, size_t pitch, uint32_t num_rows,
    const uint32_t* sources, const uint32_t* row_idx,
    const spf_edge_delta* deltas, uint32_t n_deltas);
/* Next-hop masks of `num` sources straight from a device table of uint32
 * distance rows (rows[row_of[x]] = node x's row, pitch elements apart): the
 * rule of the all-sources plans (spf_nh_rows_kernel) — bit b of NH(s, v) set
 * iff s's b-th distinct neighbour f has w(s, f) + d(f, v) == d(s, v), f
 * transit or f == v (LinkState.cpp:846-870).  Every source and every
 * neighbour of a source needs a row (row_of[x] >= 0).  Source i's V * W_i
 * words go to masks + mask_off[i] (device), W_i = ceil(nbrs(s_i) / 64) (at
 * least 1).  The repaired rows of spf_table_repair get their next hops back
 * this way.  Synchronous. */
int spf_table_nexthops(
    spf_graph* g, const uint32_t* rows, size_t pitch, const int32_t* row_of, uint32_t num,
    const uint32_t* sources, uint64_t* masks, const uint64_t* mask_off);
/* Copy distance row i of the query (uint32, as spf_query_fetch_rows) to
 * row dst_rows[i] of the device table `table` (pitch bytes apart), for every
 * query, in one kernel on the graph stream (asynchronous). */
int spf_query_scatter_rows(
    spf_query* q, const uint32_t* dst_rows, void* table, size_t pitch);

/* ---- all-nodes unicast route tables ----
 * The RouteDb of EVERY node of an area from one all-sources query, on the
 * device: for query row i (node s) and prefix p, Open/R's ECMP selection
 * (SpfSolverImpl::selectEcmpOpenr, Decision.cpp:668-712 with
 * getBestAnnouncingNodes :544-630, maybeFilterDrainedNodes :651-666,
 * getNextHopsWithMetric :1093-1179, getNextHopsThrift :1181-1271; one area,
 * LFA off, not per destination — the reference runs it per node in
 * buildRouteDb :291-542).  Output per (i, p): metric (UINT32_MAX = no route:
 * s announces p or no announcer is reachable), best (the smallest reachable
 * announcer: bestPrefixEntry's node) and a link mask over s's up links (bit
 * j = the j-th half-edge of s's CSR row, i.e. linksFromNode order): the
 * next hops of the route, each with metric `metric`. */
typedef struct spf_route_table spf_route_table;
/* `q` must be a metric query (no SPF_F_UNIT_METRIC) with SPF_F_NEXTHOPS and
 * no ignore lists; prefix p is announced by announcers[ann_offsets[p] ..
 * ann_offsets[p+1]) (node ids). */
int spf_route_table_create(
    spf_query* q, uint32_t num_prefixes, const uint32_t* ann_offsets,
    const uint32_t* announcers, spf_route_table** out);
/* flags of spf_route_table_create_ex */
#define SPF_RT_LFA 0x1u /* loop-free alternates (computeLfaPaths_, Decision.cpp:1146-1175):
                           every up link to a shortest-path or LFA next-hop node, each with
                           its own metric (spf_route_table_fetch_link_metrics); needs every
                           neighbour's row in the query (all sources) */
int spf_route_table_create_ex(
    spf_query* q, uint32_t num_prefixes, const uint32_t* ann_offsets,
    const uint32_t* announcers, uint32_t flags, spf_route_table** out);
int spf_route_table_destroy(spf_route_table* t);
/* Enqueue spf_route_table_kernel after the query's last run (asynchronous,
 * graph stream). */
int spf_route_table_run(spf_route_table* t);
int spf_route_table_elapsed_ms(spf_route_table* t, float* ms);
/* Link-mask words per prefix of row i (ceil(up links of s / 64)). */
int spf_route_table_link_words(const spf_route_table* t, uint32_t i);
/* Row i to host: metric[P], best[P], links[P * link_words(i)]. */
int spf_route_table_fetch(
    spf_route_table* t, uint32_t i, uint32_t* metric, uint32_t* best, uint64_t* links);

/* SPF_RT_LFA tables: the metric of every link of row i's source per prefix,
 * out[p * deg + j] (deg = up links of the source in CSR order), set where bit
 * j of the cell's link mask is; the diff compares these too. */
int spf_route_table_fetch_link_metrics(spf_route_table* t, uint32_t i, uint32_t* out);

/* ---- selected columns: BGP best path per node with the IGP cost ----
 * With bgpUseIgpMetric the metric-vector selection (SpfSolverImpl::
 * runBestPathSelectionBgp, Decision.cpp:714-803) differs per node: every
 * candidate's vector gets an OPENR_IGP_COST entity holding -d(node,
 * announcer) before the fold (:746-766).  compareMetricVectors(mv_i + igp_i,
 * mv_b + igp_b) depends on the two IGP values only through the sign of
 * d_i - d_b, so the caller gives three CompareResult codes per ordered pair
 * and spf_route_select_kernel folds every (row, selected column) on the
 * device, in the order of the column's announcers[] ("candidates"):
 * unreachable candidates are skipped (:726-733), the first reachable one is
 * a WINNER, igp = min d over every reachable candidate (bestIgpMetric),
 * TIE / ERROR end the fold with no route (:784-792).  Then
 * maybeFilterDrainedNodes (:651-666) on the winners through the graph's
 * node_overloaded bits, and selectEcmpBgp's (:805-866) refusals: no winner,
 * the row's node among the filtered winners, or a best candidate without
 * loopback.  The route kernel then computes the cell as for any column, over
 * the candidates in the winners word only, with `best` = the fold's best
 * candidate (not re-chosen by the drain filter). */
typedef struct spf_route_select_desc {
  uint32_t num_selected;
  const uint32_t* columns;      /* [num_selected] distinct column indices, each with at most
                                   32 announcers */
  const uint64_t* pair_offsets; /* [num_selected + 1]: column k's pair table is pair_codes[
                                   pair_offsets[k] ..), at least n(n-1)/2 entries */
  const uint16_t* pair_codes;   /* entry i(i-1)/2 + b (b < i, candidate indices): candidate i
                                   against a current best b; bits 0-2 the result when i is
                                   closer than b, 3-5 at equal distance, 6-8 when farther.
                                   Codes: 0 WINNER, 1 TIE_WINNER, 2 TIE, 3 TIE_LOOSER,
                                   4 LOOSER, 5 ERROR (6, 7 read as ERROR) */
  const uint8_t* cand_flags;    /* parallel to announcers[] (entries of unselected columns
                                   are ignored): bit 0 = the candidate has exactly one
                                   loopback via of the prefix family
                                   (PrefixState::getLoopbackVias, PrefixState.cpp:111-126) */
} spf_route_select_desc;
/* spf_route_table_create_ex with selected columns (sel NULL or empty: the
 * same table as create_ex builds, run by the same kernel instance). */
int spf_route_table_create_sel(
    spf_query* q, uint32_t num_prefixes, const uint32_t* ann_offsets,
    const uint32_t* announcers, uint32_t flags, const spf_route_select_desc* sel,
    spf_route_table** out);
/* Device time of spf_route_select_kernel in the last run (0 without selected
 * columns); spf_route_table_elapsed_ms stays the route kernel's alone. */
int spf_route_table_select_elapsed_ms(spf_route_table* t, float* ms);
/* spf_route_table_fetch plus, per column, the selection's words: igp[P]
 * (bestIgpMetric, Decision.cpp:752-755: the bestNexthop metric of
 * selectEcmpBgp :829-831) and winners[P] (bit c = candidate c of the column
 * is a next-hop destination).  Unselected columns and cells without a route
 * read igp UINT32_MAX, winners 0; in a selected column `best` is the fold's
 * best candidate.  spf_route_table_diff and _diff_mapped compare metric,
 * best and links as for any column and, in a column selected in both tables,
 * the igp word too (a cell with a route on both sides whose igp differs is
 * changed: bestNexthop.metric is part of RibUnicastEntry equality). */
int spf_route_table_fetch_sel(
    spf_route_table* t, uint32_t i, uint32_t* metric, uint32_t* best, uint64_t* links,
    uint32_t* igp, uint32_t* winners);

/* Network-wide route delta: compare two tables built
 * over graphs with the same CSR layout (e.g. before and after an overload or
 * metric change) and the same prefixes; cell (i, p) changed iff its metric,
 * best announcer or link mask differs — getRouteDelta's (Decision.cpp:47-85)
 * unicast updates and deletes for every node at once.  changed[i] = changed
 * prefixes of row i (host [num rows]); the per-row bitmap is kept in `newer`
 * (spf_route_table_changed).  SPF_E_UNSUPPORTED if the layouts differ, or if
 * the two tables do not select the same columns (spf_route_table_create_sel). */
int spf_route_table_diff(spf_route_table* older, spf_route_table* newer, uint32_t* changed);
/* SPF_RT_LFA tables: with `on` non-zero, later diffs whose `newer` is `t`
 * (spf_route_table_diff and _diff_mapped) use the metric word to tell route
 * from no route only.  Every next hop of an LFA cell has its own metric
 * (spf_route_table_fetch_link_metrics), which the diff compares link by link;
 * the cell's metric, the shortest distance, is in no next hop's place, and a
 * drained neighbour can raise it while the route stays the same.  Off by
 * default.  SPF_E_INVALID on a table without SPF_RT_LFA. */
int spf_route_table_diff_routes(spf_route_table* t, int on);
/* Changed-prefix bitmap of row i from the last diff: bits[ceil(P/64)]. */
int spf_route_table_changed(spf_route_table* t, uint32_t i, uint64_t* bits);

/* The maps of spf_route_table_diff_mapped (host arrays, read during the
 * call).  A null array is the identity map (a null dirty_off: no dirty
 * announcers); SPF_MAP_NONE marks an entry with no counterpart. */
#define SPF_MAP_NONE 0xFFFFFFFFu
typedef struct spf_route_diff_map {
  const uint32_t* row_of;    /* [newer rows]: older row, or NONE */
  const uint32_t* col_of;    /* [newer P]: older column, or NONE; injective */
  const uint32_t* gone_cols; /* [num_gone]: older columns with no newer counterpart */
  const uint32_t* node_of;   /* [older V]: newer node id, or NONE */
  const uint32_t* link_off;  /* [newer rows + 1]: offsets into link_of */
  const uint32_t* link_of;   /* per newer row, per up link in CSR order: the older row's bit
                                position, or NONE; injective within a row.  A row's segment is
                                its link count long, or empty: identity for that row (the
                                rows then have equal link counts; a newer row without links
                                has no route in any cell and goes with any older row) */
  const uint32_t* dirty_off; /* [newer P + 1]: offsets into dirty_ann */
  const uint32_t* dirty_ann; /* newer node ids: announcers of the column whose prefix entry
                                changed (a route whose best is one of them is an update).
                                An entry SPF_MAP_NONE marks a column whose best announcer is
                                no part of the route (a BGP column selected once for all
                                nodes): best is not compared in that column */
  uint32_t num_gone;
} spf_route_diff_map;
/* The route delta of every node (getRouteDelta, Decision.cpp:47-85) between
 * tables whose nodes, columns and link layouts differ (a link down or up, a
 * node joining or leaving, a prefix announced or withdrawn): cell (i, p) of
 * `newer` is compared with cell (row_of[i], col_of[p]) of `older`, link masks
 * through link_of as sets of links, best announcers through node_of.  Changed
 * iff exactly one side has a route (metric != UINT32_MAX; a cell without a
 * counterpart has none), or both have one and the metric, the mapped best,
 * the link set or (SPF_RT_LFA) a link's own metric differs, or the newer best
 * is a dirty announcer of the column.  For every gone column the older cell's
 * route is a delete (spf_route_table_changed_gone).  changed[i] = changed
 * newer columns + deleted gone columns of row i; the bitmaps are kept in
 * `newer`.  Rows whose links keep their positions compare mask words like
 * spf_route_table_diff; a remapped row may have at most 1024 links.
 * SPF_E_INVALID for an out-of-range entry, a col_of / link_of that is not
 * injective or a col_of that pairs a selected column with an unselected one,
 * SPF_E_UNSUPPORTED when the tables differ in SPF_RT_LFA or in device.  A
 * null `map` is all identity. */
int spf_route_table_diff_mapped(
    spf_route_table* older, spf_route_table* newer, const spf_route_diff_map* map,
    uint32_t* changed);
/* Deleted-column bitmap of row i from the last spf_route_table_diff_mapped
 * (the deletes of getRouteDelta, Decision.cpp:47-85): bit g set iff the older
 * row had a route in gone_cols[g]; bits[ceil(num_gone/64)]. */
int spf_route_table_changed_gone(spf_route_table* t, uint32_t i, uint64_t* bits);

/* A prefix change in place (PrefixState::updatePrefixDatabase's changed set:
 * the graph, the query's rows and the next-hop masks are as they were): the
 * listed columns of a table that has run get new announcer lists and
 * spf_route_patch_kernel recomputes their cells from the resident SPF rows,
 * comparing each with the cell it replaces in the same pass. */
typedef struct spf_route_patch {
  uint32_t num_columns;
  const uint32_t* columns;     /* [num_columns] distinct column indices < P */
  const uint32_t* ann_offsets; /* [num_columns + 1], starts at 0, monotone */
  const uint32_t* announcers;  /* node ids: the NEW announcer list of columns[k] */
  const uint32_t* dirty_off;   /* [num_columns + 1] or NULL (no dirty announcers) */
  const uint32_t* dirty_ann;   /* node ids, same meaning as spf_route_diff_map::dirty_ann */
} spf_route_patch;
/* After the call every cell of `t` is bit-equal to the cell of a table freshly
 * created over the same query with the patched announcer lists and run
 * (metric, best, link words and, SPF_RT_LFA, link metrics); columns not listed
 * are not touched.  The resident announcer arrays are replaced too: a later
 * spf_route_table_run on `t` reproduces the patched cells.
 * The changed bitmap of `t` becomes what spf_route_table_diff_mapped(before,
 * after, map) reports with all-identity maps and the given dirty lists: cell
 * (i, c) is set iff exactly one side has a route, or both have one and the
 * metric, the best announcer, the link words or (SPF_RT_LFA) a link metric
 * differs, or the new best is a dirty announcer of the column
 * (spf_route_table_diff_routes is honoured); bits of unlisted columns are
 * clear; changed[i] (NULL: not wanted) = the popcount of row i.  `t` is left as
 * after an equal-layout diff: the epoch moved (an earlier pack is stale),
 * spf_route_table_changed, _delta_pack, _delta_fetch and _fetch_cells work,
 * _changed_gone reports no gone columns, and a second patch replaces the
 * first one's bitmap.  num_columns == 0 is SPF_OK with an all-clear bitmap.
 * Everything is checked on the host first; on an error the table, its bitmap
 * and its pack state are as before the call.  SPF_E_INVALID: a null argument,
 * a table that has not run, a column >= P or listed twice, an announcer or
 * dirty id >= V (SPF_MAP_NONE included), offsets that do not start at 0 or
 * decrease.  SPF_E_UNSUPPORTED: a listed column that is a selected one (its
 * pair tables would have to be replaced: recreate the table).
 * Earlier work on the graph's stream (spf_route_table_run is asynchronous)
 * ends before the old announcer arrays are released; the call returns after
 * the patch.  The scratch cells it keeps are num_columns / P of the table's. */
int spf_route_table_patch_columns(spf_route_table* t, const spf_route_patch* p,
                                  uint32_t* changed /*[rows] or NULL*/);
/* spf_route_table_patch_columns for tables with selected columns (BGP
 * columns): `p` means what it means there; `sel` describes the listed columns
 * that are selected columns of `t`.  sel->columns holds table column indices,
 * each also in p->columns and a selected column of `t`; every listed column
 * that is selected in `t` must appear in it.  sel->pair_offsets / pair_codes
 * are the NEW pair tables of those columns (at least n(n-1)/2 entries each,
 * n <= 32 candidates), sel->cand_flags is parallel to p->announcers (entries of
 * unselected columns are ignored).  A column's kind is fixed at creation: the
 * [rows][S] selection words and the table's selected set do not move, so `sel`
 * cannot turn an unselected column into a selected one or back.  A table gets
 * spare selected columns by being created with selected columns whose
 * candidate list is empty.
 * In this call only, the dirty list of an UNSELECTED column may hold
 * SPF_MAP_NONE, with the meaning of spf_route_diff_map::dirty_ann: best is
 * not compared in that column (a BGP column selected once on the host).
 * After the call every cell of `t` is bit-equal to the cell of a table freshly
 * created over the same query with spf_route_table_create_sel, the patched
 * announcer lists, pair tables and flags, and run: metric, best, link words,
 * (SPF_RT_LFA) link metrics and what spf_route_table_fetch_sel reads, igp and
 * winners.  The resident announcer, flag, pair-offset and pair arrays are
 * replaced (later columns' offsets shift when a list changes its length): a
 * later spf_route_table_run reproduces the patched cells.
 * The changed bitmap equals what spf_route_table_diff_mapped(before, after,
 * map) reports with identity maps and the given dirty lists, its rule for a
 * column selected on both sides included: a cell with a route before and after
 * whose igp word differs is set.  spf_route_table_diff_routes is honoured.
 * `t` is left as after an equal-layout diff, as by the call above; in addition
 * spf_route_table_delta_fetch_igp and _fetch_cells_igp return the new igp
 * words.
 * Everything is checked on the host first; on an error the table, its bitmap
 * and its pack state are as before the call.  SPF_E_INVALID: everything the
 * call above rejects (but a selected column, which is accepted here); a `sel`
 * column that `p` does not list, that is not a selected column of `t` or that
 * is listed twice; a listed selected column missing from `sel`; more than 32
 * candidates; a pair table shorter than n(n-1)/2; pair_offsets[0] != 0 or
 * decreasing offsets; a null array that is needed; SPF_MAP_NONE in the dirty
 * list of a selected column.  With `sel` NULL or empty and no listed column
 * selected the call behaves as the one above, apart from the SPF_MAP_NONE
 * rule. */
int spf_route_table_patch_columns_sel(
    spf_route_table* t, const spf_route_patch* p, const spf_route_select_desc* sel,
    uint32_t* changed /*[rows] or NULL*/);
/* Device time of the last spf_route_table_patch_columns or _patch_columns_sel
 * (clearing the bitmap and spf_route_patch_kernel). */
int spf_route_table_patch_elapsed_ms(spf_route_table* t, float* ms);

/* A topology change that keeps the CSR layout (metrics patched with
 * spf_graph_patch_metrics, transit bits with spf_graph_set_transit, links taken
 * down or brought back with spf_graph_set_edges), in place:
 * `q` is an all-rows query over the SAME graph as the table's, with the same
 * sources in the same order, SPF_F_NEXTHOPS, no unit metric, no ignore lists,
 * 32-bit rows, and it has run since the graph changed.  It may be the table's
 * own query re-run, or a new one (the planner fixes a query's plan at creation:
 * spf_query_run refuses a re-run the change made stale, see there -- a metric
 * change that ends a uniform metric needs a new one).
 * After spf_graph_set_edges it must be a NEW query, created after that call:
 * the next-hop mask bits follow the distinct-neighbour lists, which the call
 * rebuilds (the mask widths may differ from the table's old query; an
 * SPF_RT_LFA table still needs every source within 256 neighbours, else
 * SPF_E_UNSUPPORTED).  The cells do not move: a link bit and a link metric are
 * indexed by CSR position, a down half-edge keeps its position, never has a
 * bit, and has link metric UINT32_MAX; spf_route_table_link_words and the
 * link-metric row length stay those of the CSR row, down slots included.
 * spf_route_refresh_kernel recomputes every cell of the listed rows from q's
 * rows and masks and compares each with the cell it replaces in the same pass.
 * After the call every cell of a listed row is bit-equal to the cell of a table
 * freshly created over `q` with the table's announcer lists and flags, and run
 * (metric, best, link words and, SPF_RT_LFA, link metrics).  Rows not listed
 * are neither read nor written: the caller vouches that their SPF rows, masks,
 * own link metrics and (SPF_RT_LFA) neighbours' rows are as before; the call
 * does not check it.
 * The changed bitmap of `t` becomes what spf_route_table_diff(before, after)
 * reports for the listed rows (spf_route_table_diff_routes is honoured);
 * unlisted rows are clear; changed[i] (NULL: not wanted) = the popcount of row
 * i.  `t` is left as after an equal-layout diff: the epoch moved (an earlier
 * pack is stale), spf_route_table_changed, _delta_pack, _delta_fetch and
 * _fetch_cells work, _changed_gone reports no gone columns, a later
 * _patch_columns or _refresh_rows replaces the bitmap, and a later
 * spf_route_table_run reproduces the same cells from `q`.
 * The table is bound to `q` from then on and the user counts of the lifetime
 * rule move with it: the old query can be destroyed, `q` cannot while `t`
 * lives (SPF_E_INVALID).
 * Everything is checked on the host first; on an error the table, its bitmap,
 * its pack state and its query binding are as before the call.
 * SPF_E_INVALID: a null `t` or `q`, a table or a `q` that has not run, a `q`
 * over another graph, with other sources, without next hops, with unit metric
 * or ignore lists, a row >= the table's rows or listed twice.
 * SPF_E_UNSUPPORTED: 64-bit rows; a table with selected columns (BGP columns:
 * their selection words follow the rows too -- spf_route_table_refresh_rows_sel
 * below takes those).  num_rows == 0 with a non-null
 * `rows` is SPF_OK: the bitmap is all clear and the binding moves.
 * Memory: the cells the call replaces are kept in a previous-cell store of the
 * listed rows' size (grow-only; with every row listed one more cell store).
 * No second graph, no second rows or masks and no host maps are needed. */
int spf_route_table_refresh_rows(
    spf_route_table* t, spf_query* q,
    uint32_t num_rows, const uint32_t* rows /* distinct, < nq; NULL: every row */,
    uint32_t* changed /*[rows of t] or NULL*/);
/* Device time of the last spf_route_table_refresh_rows (clearing the bitmap
 * and spf_route_refresh_kernel). */
int spf_route_table_refresh_elapsed_ms(spf_route_table* t, float* ms);
/* The cells as they were before the last refresh: spf_route_table_fetch_cells'
 * arguments and packing; any (row, column), listed in that refresh or not (a
 * listed row's cells come from the store, the others are the resident ones).
 * What getRouteDelta's MPLS side needs without an older table: the entry of a
 * label before the change, from cells of label columns that may not have
 * changed.  Answers until the next run, patch or refresh of `t`;
 * SPF_E_INVALID when no refresh is current. */
int spf_route_table_fetch_cells_prev(
    spf_route_table* t, uint64_t n, const uint32_t* rows, const uint32_t* cols,
    uint32_t* metric, uint32_t* best, uint64_t* links, uint32_t* link_metrics);
/* spf_route_table_refresh_rows for tables with selected columns
 * (spf_route_table_create_sel): same arguments, same host-side checks (without
 * the selected-columns refusal), same epoch, pack state, query binding and
 * error behaviour -- on any error nothing is touched.  On a table without
 * selected columns it IS that call (same kernel instance, same bitmap).
 * For a selected column nothing the host handed over depends on the topology:
 * spf_route_refresh_kernel<true> folds the column's resident candidate list
 * with its resident pair table and candidate flags (those of create_sel or of
 * the last _patch_columns_sel) over q's row of the node and the graph's
 * current transit bits, then computes the cell over the winners word, as
 * spf_route_patch_kernel<.., true> does per column.  After the call every
 * listed row is bit-equal to a table freshly created over `q` with
 * spf_route_table_create_sel and the table's current lists, pair tables and
 * flags, and run: metric, best, link words, SPF_RT_LFA link metrics and the
 * selection words (igp and winners, spf_route_table_fetch_sel).  A cell with a
 * route before and after whose igp word differs is changed too, so the bitmap
 * is spf_route_table_diff(before, after) of two such tables on the listed rows.
 * spf_route_table_delta_pack / _delta_fetch_igp and _fetch_cells_igp return the
 * new igp words; a later _patch_columns_sel or spf_route_table_run works as
 * after _refresh_rows.  Memory: the store also keeps the listed rows' previous
 * igp words ([listed rows][selected columns], grow-only). */
int spf_route_table_refresh_rows_sel(
    spf_route_table* t, spf_query* q,
    uint32_t num_rows, const uint32_t* rows /* distinct, < nq; NULL: every row */,
    uint32_t* changed /*[rows of t] or NULL*/);
/* The igp words as they were before the last refresh, for any (row, column):
 * a listed row's come from the store, the others are the resident ones;
 * UINT32_MAX in an unselected column.  SPF_E_UNSUPPORTED on a table without
 * selected columns; SPF_E_INVALID when no refresh is current. */
int spf_route_table_fetch_cells_prev_igp(
    spf_route_table* t, uint64_t n, const uint32_t* rows, const uint32_t* cols, uint32_t* igp);

/* The delta itself (getRouteDelta, Decision.cpp:47-85: the updates and
 * deletes, not their number) of every node as one record list built on the
 * device: the changed cells of the last diff, compacted out of the bitmaps,
 * so that a consumer copies the cells that changed and not two whole rows per
 * node.  Compute on the device, then fetch (as spf_query_trace_paths /
 * _trace_fetch). */
typedef struct spf_route_delta_sizes {
  uint64_t cells;        /* changed cells of `newer` over all rows */
  uint64_t gone;         /* deleted gone-column entries over all rows */
  uint64_t link_words;   /* sum over changed cells of link_words(row) */
  uint64_t link_metrics; /* SPF_RT_LFA: sum over changed cells of deg(row); else 0 */
} spf_route_delta_sizes;
/* After spf_route_table_diff or _diff_mapped on `newer`: build, on the device,
 * the list of its changed cells.  Rows ascending; columns ascending within a
 * row.  The values are copies taken from `newer` alone (`older` is not needed
 * after the call); the buffers belong to the table and only grow.  After an
 * equal-layout diff `gone` is 0.  SPF_E_INVALID before any diff (or after a
 * later spf_route_table_run with no diff since); zero changed cells is
 * SPF_OK with all sizes 0.  Synchronises the graph stream once. */
int spf_route_table_delta_pack(spf_route_table* newer, spf_route_delta_sizes* sizes);
/* The packed list to host.  Cell k of row i has cell_off[i] <= k <
 * cell_off[i+1]; its link words start at sum over r<i of (cell_off[r+1] -
 * cell_off[r]) * link_words(r) + (k - cell_off[i]) * link_words(i), its link
 * metrics (SPF_RT_LFA) at the same sum with deg(row) in place of link_words
 * (a row without up links has cells and no link words).  gone[] holds indices
 * g into the diff's gone_cols, row i's in gone_off[i] .. gone_off[i+1].
 * SPF_E_INVALID before a pack, or when the table ran or diffed since (the
 * pack is stale). */
int spf_route_table_delta_fetch(
    spf_route_table* newer,
    uint64_t* cell_off /*[rows+1]*/, uint32_t* col, uint32_t* metric, uint32_t* best /*[cells]*/,
    uint64_t* links /*[link_words]*/, uint32_t* link_metrics /*[link_metrics], NULL unless LFA*/,
    uint64_t* gone_off /*[rows+1]*/, uint32_t* gone /*[gone]: index g into gone_cols*/);
/* Tables with selected columns: the pack also copies every changed cell's igp
 * word (UINT32_MAX in an unselected column, as spf_route_table_fetch_sel
 * reads), in the packed list's order.  Same staleness rules as
 * spf_route_table_delta_fetch; SPF_E_UNSUPPORTED on a table without selected
 * columns. */
int spf_route_table_delta_fetch_igp(spf_route_table* newer, uint32_t* igp /*[cells]*/);
/* Sparse read of any run table: cell k = (rows[k], cols[k]) (repeats allowed).
 * Links and link metrics are packed in list order, link_words(rows[k]) /
 * deg(rows[k]) each (link_metrics: SPF_RT_LFA tables only, else NULL).  What
 * getRouteDelta's MPLS side needs of a column that did not change.  Rows and
 * columns are checked on the host before any launch (SPF_E_INVALID); n = 0 is
 * SPF_OK. */
int spf_route_table_fetch_cells(
    spf_route_table* t, uint64_t n, const uint32_t* rows, const uint32_t* cols,
    uint32_t* metric, uint32_t* best, uint64_t* links, uint32_t* link_metrics);
/* The igp word of the same kind of list (UINT32_MAX in an unselected column).
 * Same checks as spf_route_table_fetch_cells; SPF_E_UNSUPPORTED on a table
 * without selected columns. */
int spf_route_table_fetch_cells_igp(
    spf_route_table* t, uint64_t n, const uint32_t* rows, const uint32_t* cols, uint32_t* igp);

/* ---- multi-GPU all-sources tables ----
 * The reference computes every SpfResult on the one Decision thread
 * (getSpfResult, LinkState.cpp:791-801; all sources = Decision::
 * getDecisionRouteDb per node, Decision.cpp:1437-1462).  Here one call fans
 * an all-sources batch out over devices: sources are split in contiguous
 * blocks (rank r of `world`: n / world sources, the first n % world ranks one
 * more), each block runs as one spf_query on its device, and the rows are
 * exchanged with an in-place RCCL all-gather over xGMI into equal-sized rank
 * slots.  A cluster is either every device of this process
 * (spf_cluster_create_local: ncclCommInitAll) or one rank of a
 * one-process-per-GPU job (spf_cluster_create_rank: ncclCommInitRank over an
 * id from spf_cluster_unique_id that the caller hands to every rank). */
typedef struct spf_cluster spf_cluster;
typedef struct spf_table spf_table;

#define SPF_CLUSTER_ID_BYTES 128
#define SPF_T_GATHER_ROWS 0x100u     /* all-gather the uint32 distance rows */
#define SPF_T_GATHER_NEXTHOPS 0x200u /* all-gather the packed next-hop masks */
/* All-gather the distance rows as 8-bit LEVEL rows, a quarter of the uint32
 * bytes: on a uniform metric (or SPF_F_UNIT_METRIC) the MS-BFS plan's level
 * byte encodes a distance exactly (distance = level * scale, 255 = not
 * reached) while no level reaches 255.  Allowed with SPF_T_GATHER_NEXTHOPS;
 * with SPF_T_GATHER_ROWS it is SPF_E_INVALID.  Creation refuses it with
 * SPF_E_UNSUPPORTED only for facts of the graph, equal on every rank, that
 * rule the MS-BFS plan out for good (a metric that is not uniform without
 * SPF_F_UNIT_METRIC, more nodes than the plan holds); what depends on a
 * rank's block or on a run is decided per run:
 *   - spf_table_run copies each local block's level rows into its slot
 *     (spf_query_pack_levels; layout: spf_table_levels_layout) and exchanges
 *     the slots with ONE in-place all-gather of slot_bytes bytes; no uint32
 *     row is copied or exchanged.
 *   - The run is RESOLVED in spf_table_sync (and implicitly by any reader of
 *     gathered data, and by spf_table_row_form / spf_table_elapsed_ms, when
 *     the last run is unresolved): the `world` trailers are read from one
 *     local device.  All flags words 0: the run's form is LEVELS.  Otherwise
 *     (a deep BFS, or a block without level rows) it is ROWS32, the fallback:
 *     the uint32 gathered buffer is allocated (once), each block's rows are
 *     copied into its slot and all-gathered exactly as SPF_T_GATHER_ROWS
 *     does.  Every rank reads the same trailers and so takes the same branch,
 *     but the fallback is a collective: for such a table spf_table_sync (and
 *     the first reader after a run) is COLLECTIVE -- every rank must call it
 *     after every run.  The form is decided anew on every run (a drain can
 *     make a BFS deep or shallow again).  A block on a 64-bit plan fails
 *     the fallback with SPF_E_UNSUPPORTED, as a SPF_T_GATHER_ROWS run does.
 *   - Readers return the same uint32 rows in either form. */
#define SPF_T_GATHER_LEVELS 0x400u

int spf_cluster_unique_id(uint8_t* id /*[SPF_CLUSTER_ID_BYTES]*/);
int spf_cluster_create_local(uint32_t num_devices, const int* devices, spf_cluster** out);
int spf_cluster_create_rank(
    uint32_t world, uint32_t rank, const uint8_t* id, int device, spf_cluster** out);
int spf_cluster_destroy(spf_cluster* c);
int spf_cluster_info(
    const spf_cluster* c, uint32_t* world, uint32_t* first_rank, uint32_t* local_devices);
const char* spf_cluster_last_error(void);

/* Host only: the block boundaries (block_first[world + 1]) and, when
 * mask_off is non-NULL, the BYTE offset of every source's next-hop masks in
 * the gathered mask buffer (rank slots of *mask_cap bytes; within a slot the
 * block's sources back to back, V * nh_bytes[i] bytes each rounded up to 32:
 * the device layout of spf_query_nh_bytes / SPF_NH_BYTES).  nh_bytes may be
 * NULL (8 bytes = one word each). */
int spf_table_layout(
    uint32_t num_sources, uint32_t world, uint32_t num_nodes, const uint32_t* nh_bytes,
    uint64_t* block_first, uint64_t* mask_off, uint64_t* mask_cap);
/* Host only: the level slots of a SPF_T_GATHER_LEVELS table.  Each of the
 * `world` equal slots of *slot_bytes bytes (a multiple of 16) holds cap =
 * ceil(num_sources / world) level rows *pitch bytes apart (*pitch = num_nodes
 * rounded up to 16, the level-row stride of a query, so a block's rows are
 * one contiguous run; the bytes [num_nodes, pitch) of a row are padding) and,
 * *trailer_off = cap * pitch bytes into the slot, the block's 16-byte trailer
 * (spf_query_pack_levels; all zero for a rank with an empty block).  Source i
 * of rank r's block (spf_table_layout's block_first) is at r * slot_bytes +
 * (i - block_first[r]) * pitch.  Any output pointer may be NULL, not all. */
int spf_table_levels_layout(
    uint32_t num_sources, uint32_t world, uint32_t num_nodes, uint64_t* pitch,
    uint64_t* slot_bytes, uint64_t* trailer_off);
/* One graph per local device from `desc` (desc->device ignored), the local
 * ranks' source blocks as queries.  flags: SPF_F_UNIT_METRIC,
 * SPF_F_NEXTHOPS, SPF_T_GATHER_ROWS, SPF_T_GATHER_NEXTHOPS,
 * SPF_T_GATHER_LEVELS. */
int spf_table_create(
    spf_cluster* c, const spf_graph_desc* desc, uint32_t num_sources, const uint32_t* sources,
    uint32_t flags, spf_table** out);
int spf_table_destroy(spf_table* t);
/* Enqueue every local block and the all-gathers (asynchronous). */
int spf_table_run(spf_table* t);
/* Wait for the last run (and for spf_table_expand_rows calls since).  For a
 * SPF_T_GATHER_LEVELS table it also resolves the run's form and is
 * COLLECTIVE (see the flag). */
int spf_table_sync(spf_table* t);
/* Device time of the last run, max over local devices: the SPF batch (plus
 * the copy into the own slot) and the RCCL exchange (a SPF_T_GATHER_LEVELS
 * run's fallback exchange included). */
int spf_table_elapsed_ms(spf_table* t, float* compute_ms, float* gather_ms);
int spf_table_block(const spf_table* t, uint32_t rank, uint32_t* first, uint32_t* count);
int spf_table_nh_words(const spf_table* t, uint32_t i);
/* Device bytes per node of source i's masks in the gathered buffer. */
int spf_table_nh_bytes(const spf_table* t, uint32_t i);
/* Rows / masks of sources [first, first+count) to host memory (from the
 * local owner, or from the gathered copy; SPF_E_UNSUPPORTED for another
 * rank's rows without the gather flag).  With SPF_T_GATHER_LEVELS another
 * rank's rows are expanded on the device (spf_table_expand_rows' routine, a
 * bounded scratch) and copied from there.  Masks back to back, V * nh_words(i)
 * words each. */
int spf_table_fetch_rows(spf_table* t, uint32_t first, uint32_t count, uint32_t* dst);
int spf_table_fetch_nexthops(spf_table* t, uint32_t first, uint32_t count, uint64_t* dst);
/* SPF_T_GATHER_LEVELS readers (all resolve an unresolved run first).
 * spf_table_row_form: *form = SPF_ROW_FORM_* of the last run (a table without
 * the flag: ROWS32 with SPF_T_GATHER_ROWS, else NONE), *scale = the level
 * scale (LEVELS form, else 0), *gathered_bytes = the bytes each rank received
 * in the last run's row exchange (LEVELS: world * slot_bytes; the fallback
 * adds world * cap * V * 4).  Outputs may be NULL. */
#define SPF_ROW_FORM_NONE 0u
#define SPF_ROW_FORM_ROWS32 1u
#define SPF_ROW_FORM_LEVELS 2u
int spf_table_row_form(spf_table* t, uint32_t* form, uint32_t* scale, uint64_t* gathered_bytes);
/* The uint32 rows of sources [first, first+count) into device memory of
 * local device `local` (dst_pitch >= 4 * V bytes apart, dst and dst_pitch
 * multiples of 4; V entries written per row, nothing else), FROM THE GATHERED
 * BUFFER of that device, whoever owns the sources: spf_levels_expand_kernel
 * in LEVELS form, a strided copy in ROWS32 form (also a SPF_T_GATHER_ROWS
 * table's).  Asynchronous on that device's graph stream; spf_table_sync
 * waits for it.  SPF_E_UNSUPPORTED for a table without a row gather. */
int spf_table_expand_rows(
    spf_table* t, uint32_t local, uint32_t first, uint32_t count, void* dst_dev,
    size_t dst_pitch);
/* The raw level bytes of sources [first, first+count) from the gathered
 * buffer to host memory, [count][V]; SPF_E_UNSUPPORTED unless the last run's
 * form is LEVELS. */
int spf_table_fetch_levels(spf_table* t, uint32_t first, uint32_t count, uint8_t* dst);
/* The gathered level slots on local device `local` ([world * slot_bytes]
 * bytes, spf_table_levels_layout; NULL without SPF_T_GATHER_LEVELS), valid
 * data only after a run whose form is LEVELS.  Like
 * spf_table_device_buffers it needs no run. */
int spf_table_levels_buffer(
    spf_table* t, uint32_t local, void** levels, uint64_t* pitch, uint64_t* slot_bytes);
/* spf_query_trace_paths over every local block of the table (each block on
 * its device, concurrently); dests and the counts are indexed by table
 * query.  Other ranks' blocks are not traced (their counts are 0).  Then
 * spf_table_trace_fetch packs the local blocks' paths in table-query order,
 * as spf_query_trace_fetch does. */
int spf_table_trace_paths(
    spf_table* t, const uint32_t* dests, uint32_t* path_count, uint32_t* link_count);
int spf_table_trace_fetch(spf_table* t, uint32_t* links, uint32_t* ends);
/* spf_query_trace_expand / _expand_fetch over every local block, after
 * spf_table_trace_paths; costs and labels packed in table-query order. */
int spf_table_trace_expand(spf_table* t, const int32_t* node_labels);
int spf_table_trace_expand_fetch(spf_table* t, uint64_t* cost, int32_t* labels);
/* Gathered buffers on local device `local`: rows [world * cap][V] uint32
 * (cap = ceil(n / world)), masks [world * mask_cap] bytes in the layout of
 * spf_table_layout; NULL when that gather is off (a SPF_T_GATHER_LEVELS
 * table: rows is NULL until a run fell back to ROWS32 and the buffer exists;
 * its content is current only while spf_table_row_form says ROWS32). */
int spf_table_device_buffers(
    spf_table* t, uint32_t local, void** rows, void** masks, uint64_t* mask_cap_bytes);
int spf_table_kernel_name(spf_table* t, uint32_t local, const char** name);

/* ---- persistent cluster graphs + query tables ----
 * One spf_graph per local device of a cluster, created once per area and
 * topology and kept across batches (the host LinkState patches it with the
 * same overload / metric churn as its single-device graph), instead of one
 * graph upload per device per table.  Over it, spf_table_create_q shards ANY
 * query batch -- with per-query ignore lists -- over the ranks in contiguous
 * blocks: KSP2 second passes by destination (LinkState::getKthPaths k = 2,
 * runSpf(src, true, linksToIgnore) at LinkState.cpp:776-777), what-if by
 * failed link (runSpf with linksToIgnore, LinkState.cpp:842-847), LFA by
 * neighbour (getSpfResult per neighbour, Decision.cpp:1145-1174). */
typedef struct spf_cgraph spf_cgraph;
int spf_cgraph_create(spf_cluster* c, const spf_graph_desc* desc, spf_cgraph** out);
int spf_cgraph_destroy(spf_cgraph* g);
int spf_cgraph_set_transit(spf_cgraph* g, const uint8_t* node_overloaded);
int spf_cgraph_patch_metrics(
    spf_cgraph* g, uint32_t n, const uint32_t* edge_idx, const uint64_t* metric);
/* The graph of local device `local` (NULL if out of range), e.g. for
 * spf_graph_num_nbrs / spf_graph_nbrs. */
spf_graph* spf_cgraph_device_graph(spf_cgraph* g, uint32_t local);
/* A table over `g` from a full query description: desc->sources /
 * ignore_offsets / ignore_links as in spf_query_create (offsets of the whole
 * batch; each rank's block gets its slice), desc->flags SPF_F_UNIT_METRIC /
 * SPF_F_NEXTHOPS, plus the SPF_T_GATHER_* bits in `flags`.  The table
 * borrows the graphs (destroy the table before the cgraph).  Rows of 64-bit
 * plans (spf_table_fetch_rows -> SPF_E_UNSUPPORTED) are left to the caller's
 * single-device path. */
int spf_table_create_q(
    spf_cgraph* g, const spf_query_desc* desc, uint32_t flags, spf_table** out);

#ifdef __cplusplus
}
#endif

#endif /* OPENR_SPF_H */
