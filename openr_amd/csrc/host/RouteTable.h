// RouteTable.h — the unicast RouteDb of EVERY node of an area, on the device
// (SURVEY.md §8(f) row 1).
//
// The reference builds one node's RouteDb at a time on the Decision thread
// (SpfSolverImpl::buildRouteDb, openr/decision/Decision.cpp:291-542); views
// of other nodes' routes (ctrl getRouteDbComputed, OpenrCtrlHandler.cpp:
// 411-416; breeze `decision routes --nodes`, commands/decision.py:48-363)
// call it again per node.  AllNodesRouteTable runs ONE all-sources SPF with
// next hops over the area graph and spf_route_table_kernel over every
// eligible prefix, so the routes of any node are a row read away.
//
// Scope (what the kernel restates, include/openr_spf.h): prefixes advertised
// in this area only, forwarding type IP with algorithm SP_ECMP
// (Decision.cpp:395-412), v4 prefixes only with enableV4 —
// i.e. SpfSolverImpl::selectEcmpOpenr, and with bgpColumns selectEcmpBgp for
// prefixes whose entries are all BGP with a metric vector: selected once on
// the host without bgpUseIgpMetric, per node on the device with it
// (spf_route_select_kernel).  routes(node) equals the unicast entries
// SpfSolver::buildRouteDb(node) produces for those prefixes
// (tests/test_route_table.py, tests/test_route_table_bgp_igp_gpu.py).
//
// MPLS (Decision.cpp:415-534, this area, LFA off): every (node label, owner)
// pair is one more column of the same kernel pass -- a pseudo-prefix
// announced by the owner alone, so its cell is getNextHopsWithMetric(node,
// {owner}) -- and mplsRoutes(node) turns the cells into POP_AND_LOOKUP (own
// label) / PHP (next hop is the owner) / SWAP routes with the reference's
// collision rule (the smallest-named owner the node itself is or reaches),
// then adds the PHP routes of the node's adjacency labels (a node label
// keeps its entry when an adjacency label repeats it).
//
// The table owns its device graph, query and rows (a snapshot): it stays
// valid across later LinkState changes and answers for the topology it was
// built from, or the one its last applyTopologyChanges was given.
#pragma once

#include <algorithm>
#include <map>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "LinkState.h"
#include "PrefixState.h"
#include "SpfSolver.h"
#include "openr_spf.h"

namespace openr {

// The rows spf_route_table_refresh_rows must list after a metric change that
// keeps the CSR layout (row / col: the CSR; affected[i]: spf_table_screen's
// answer for node i's SPF row; changedTails: the tails of the half-edges whose
// metric differs).  Without LFA the affected rows; with it also every row with
// an affected neighbour and the tails themselves -- an LFA cell reads the
// metric of every own link and the neighbours' rows.  Ascending, host only.
std::vector<uint32_t> routeRefreshRowList(
    const std::vector<uint8_t>& affected, const std::vector<uint32_t>& row,
    const std::vector<uint32_t>& col, const std::vector<uint32_t>& changedTails, bool lfa);

class AllNodesRouteTable {
 public:
  // computeLfa: SpfSolver's computeLfaPaths (loop-free alternates as extra
  // next hops with their own metrics, Decision.cpp:1146-1175)
  // borderNodes (multi-area, see AllAreasRouteTable): non-null selects the
  // prefixes this area's table can serve for its interior nodes -- entries
  // in this area, none of them by a border node; the announcers are the
  // in-area entries (for an interior node every other area's announcer is
  // unreachable, Decision.cpp:555-579)
  // bgpColumns (round 6, AllAreasRouteTable without bgpUseIgpMetric): BGP
  // prefixes on the device too.  With no IGP metric in the vector and every
  // in-graph announcer reachable from every node, the metric-vector
  // selection (runBestPathSelectionBgp, Decision.cpp:714-803) has the same
  // winners for every node, so it runs once on the host and the kernel takes
  // the winners (drained filter applied) as the column's announcers; a node
  // among them gets no route (selectEcmpBgp :805-866).  bestPrefixEntry,
  // bestArea and the loopback next hop are the selection's; doNotInstall =
  // bgpDryRun.  A prefix with an announcer some node cannot reach stays on
  // the host.
  // bgpUseIgpMetric (with bgpColumns): the selection differs per node --
  // every candidate's vector gets an OPENR_IGP_COST entity holding -d(node,
  // announcer) before the fold (Decision.cpp:746-766) -- so a BGP prefix
  // becomes a SELECTED column: its in-graph announcers in fold order
  // (without those advertising OPENR_IGP_COST, :735-744) are the candidates,
  // compareMetricVectors runs on the host three times per ordered pair
  // (MetricVectorUtils::bgpIgpPairCodes: the result depends on the IGP
  // values only through the sign of their difference) and
  // spf_route_select_kernel folds every (node, column) from the node's own
  // distance row, skipping unreachable candidates -- no all-reachable
  // requirement, split graphs are served.  bestPrefixEntry is the cell's
  // best candidate's, bestNexthop its loopback with metric = the cell's igp.
  // spareColumns: that many extra columns with empty announcer lists, after
  // the node-label columns (every other column keeps its index), for
  // applyPrefixChanges to give to prefixes announced later.  An empty column
  // has no route in any row; with 0 the table is what it was.
  // Left to the host: more than 32 candidates, a candidate vector with a
  // foreign entity of priority 3500 (its order against the IGP entity is
  // std::sort's), entries in another area.
  // bgpInPlace (with bgpColumns): applyPrefixChanges serves BGP columns too
  // (spf_route_table_patch_columns_sel).  Off by default only because a test
  // pins the refusal of bgpColumns tables.
  // spareSelectedColumns (with bgpUseIgpMetric, else ignored): that many empty
  // SELECTED columns after the spare columns, for BGP prefixes announced later
  // (a column's kind is fixed when the device table is created).
  // linksInPlace: applyTopologyChanges also follows links that go down or come
  // back (an adjacency withdrawn or announced again, a link overload bit), see
  // there.  Off by default only because a test pins the refusal of a removed
  // link.
  AllNodesRouteTable(
      const LinkState& ls, const PrefixState& ps, bool enableV4 = true, bool computeLfa = false,
      const std::unordered_set<std::string>* borderNodes = nullptr, bool bgpColumns = false,
      bool bgpDryRun = false, bool bgpUseIgpMetric = false, size_t spareColumns = 0,
      bool bgpInPlace = false, size_t spareSelectedColumns = 0, bool linksInPlace = false);
  ~AllNodesRouteTable();
  AllNodesRouteTable(const AllNodesRouteTable&) = delete;
  AllNodesRouteTable& operator=(const AllNodesRouteTable&) = delete;

  size_t numNodes() const { return names_.size(); }
  size_t numPrefixes() const { return prefixes().size(); }
  // device time of the all-sources SPF (+ next hops) and of the route kernel
  float spfMs() const { return spfMs_; }
  float routeMs() const { return routeMs_; }
  // device time of spf_route_select_kernel (0 without selected columns)
  float selectMs() const { return selectMs_; }
  // routes present in the table (metric != no-route), over all nodes
  uint64_t countRoutes() const;

  // The unicast routes of `node` (empty if the node is not in the area).
  std::unordered_map<thrift::IpPrefix, RibUnicastEntry> routes(const std::string& node) const;
  // The MPLS routes of `node` (node labels + adjacency labels, see above).
  std::unordered_map<int32_t, RibMplsEntry> mplsRoutes(const std::string& node) const;
  size_t numLabelColumns() const { return owners_.size(); }

  // Network-wide route delta against an older table: per node of THIS table
  // (id order, see nodeName) the number of changed columns -- unicast
  // prefixes and node-label columns, deleted ones included (changedSplit
  // separates them).  Over the same graph layout, prefixes and node labels
  // this is spf_route_table_diff.  Otherwise (links down or up, nodes joined
  // or gone, prefixes announced or withdrawn, labels changed) the tables are
  // compared through maps (spf_route_table_diff_mapped): rows and best
  // announcers by node name, unicast columns by prefix, label columns by
  // (label, owner name), link bits by Link identity -- a link whose next-hop
  // addresses, interface or area (what materialise reads) differ has no
  // counterpart, so every route over it is changed -- and announcers whose
  // PrefixEntry differs are the column's dirty list.  A node the older table
  // lacks has every route changed.
  // BGP columns are compared like any other, plus what their routes hold
  // beyond the cell: in a selected column the cell's igp word
  // (bestNexthop.metric: the device diff compares it) and each candidate's
  // entry and loopback (dirty when they differ); in a host-selected column
  // the selection's best entry and loopback (every announcer dirty when they
  // differ; the cell's own best is not compared).  Any such difference, other
  // candidates or pair codes go through the maps.  A prefix whose column
  // kind differs between the tables (Open/R, host-selected, selected) has no
  // counterpart: the older column is gone and a node with a route on both
  // sides gets one update.
  // LFA tables: the cell's metric word (the shortest distance) is no part of
  // a route whose next hops carry their own metrics, so the table asks the
  // device diff to leave it out (spf_route_table_diff_routes): a drained
  // neighbour can raise it while every link keeps its bit and its metric.
  // Throws std::invalid_argument for different areas, LFA modes, bgpColumns,
  // bgpDryRun or bgpUseIgpMetric.
  std::vector<uint32_t> diff(const AllNodesRouteTable& older);
  // (changed unicast prefixes, changed node-label columns) of `node` from
  // the last diff; .first == unicast updates + deletes of delta(node)
  std::pair<uint32_t, uint32_t> changedSplit(const std::string& node) const;
  // getRouteDelta({routes, mplsRoutes}(node), the same of `older`; {} for a
  // node `older` lacks) (Decision.cpp:47-85) from the last diff: changed
  // routes materialised, vanished ones (gone columns included) deleted.  MPLS
  // candidates are the labels of changed and gone label columns, the node's
  // own label and its adjacency labels in both tables, compared entry by
  // entry against `older` (which must outlive this call).
  DecisionRouteUpdate delta(const std::string& node) const;
  // delta(nodeName(i)) for every node i of this table, in id order, from ONE
  // packed fetch instead of two whole rows per node: the changed cells are
  // compacted on the device (spf_route_table_delta_pack), unicast routes are
  // materialised straight from them, and the cells MPLS candidates need of
  // columns that did not change (every column of a candidate label, in both
  // tables) come from one spf_route_table_fetch_cells per table.  Entry i
  // holds the updates and deletes of delta(nodeName(i)); the order inside the
  // four lists is free.  Nodes are assembled on the host worker pool.
  // `older` must outlive this call.
  std::vector<DecisionRouteUpdate> deltas() const;
  // the last deltas(): wall time of its steps, the packed sizes, the cells
  // gathered from either table and the bytes copied from the device (with
  // selected columns the packed list has a fourth lane, the cells' igp)
  struct DeltasStats {
    double packUs = 0, fetchUs = 0, gatherUs = 0, assembleUs = 0, totalUs = 0;
    uint64_t cells = 0, gone = 0, linkWords = 0, linkMetrics = 0;
    uint64_t newerCells = 0, olderCells = 0, bytes = 0;
  };
  const DeltasStats& lastDeltas() const { return lastDeltas_; }
  // bytes delta(node) copies from the device for a node with a changed cell
  // and an MPLS candidate (its bitmaps, its whole row and the older table's),
  // counted from shapes on the host
  uint64_t deltaFetchBytes(const std::string& node) const;
  // wall time of the device diff call inside the last diff() (maps excluded)
  float diffCallMs() const { return diffCallMs_; }
  // the last diff() went through the maps
  bool diffWasMapped() const { return mapped_; }
  const std::string& nodeName(uint32_t id) const { return names_.at(id); }
  // the unicast prefixes the kernel serves (routes() covers exactly these)
  // (after applyPrefixChanges: without the free columns, with the spare ones in use)
  const std::vector<thrift::IpPrefix>& prefixes() const { return holes_ ? served_ : prefixes_; }

  // Prefix changes in place (PrefixState::updatePrefixDatabase's changed
  // sets, several merged if wanted; `ps` is the state now).  The topology is
  // this table's: the one it was built from, or the one of its last
  // applyTopologyChanges.  Every changed prefix is rescanned by the constructor's
  // rules (scanPrefix) and, all in ONE spf_route_table_patch_columns:
  //   served before and now: its column gets the new announcers (announcers
  //     on both sides whose PrefixEntry differs are the column's dirty list);
  //   served before, not now (withdrawn, no longer IP / SP_ECMP): the column
  //     gets an empty list and becomes free;
  //   served now, not before: it takes a free column -- one freed by an
  //     earlier call first, else a spare one.  Too few: std::length_error
  //     before anything is touched (rebuild the table).
  // Throws std::invalid_argument, before anything is touched, on a table built
  // with borderNodes, or with bgpColumns and without bgpInPlace (without
  // bgpColumns a BGP prefix is not served and takes no column).
  // bgpInPlace: a host-selected BGP column gets the new selection's winners
  // (SPF_MAP_NONE in its dirty list: best is not compared; every announcer
  // dirty when the best entry or loopback differs), a selected column its new
  // candidates, pair codes and loopback flags (candidates whose entry or
  // loopback differs are dirty) -- new ones in a free selected column.  A
  // prefix whose kind changes between unselected kinds keeps its column (every
  // announcer dirty); between a selected and an unselected column it moves,
  // and a node with a route on both sides gets one update.  In a selected
  // column best (its entry and loopback) is part of the route: a cell whose
  // best alone moved is left out only where the old and the new best
  // candidate have equal entries and equal loopbacks and the igp word stayed.  Afterwards prefixes(), routes(), countRoutes() describe the
  // new state and changedSplit / delta / deltas the delta of this call, from
  // the new cells alone (no older table; the MPLS lists are empty: label
  // columns do not move).  A cell whose best announcer alone moved, between
  // announcers with equal PrefixEntries, is no route change and is left out.
  // Returns the changed routes per node, id order.
  std::vector<uint32_t> applyPrefixChanges(
      const PrefixState& ps, const std::unordered_set<thrift::IpPrefix>& changed);
  // Topology changes that keep the CSR layout, in place: link metrics and
  // node overload (drain) bits, the common churn.  `ls` is the area's
  // LinkState now.  Throws std::invalid_argument before anything is touched
  // for a table built with borderNodes, with bgpColumns and without
  // bgpInPlace, or with bgpColumns and without bgpUseIgpMetric (host-selected
  // BGP columns depend on the drain filter and on reachability, and the cached
  // reachability answers would go stale), ls.engine().exact,
  // another area, node names, CSR row / col / rev / link ids or Link identities
  // that differ from the table's (a link down or up, a node joined or gone:
  // those need a fresh table and the mapped diff), or a node label that
  // differs (the label columns would move).  Otherwise: the edge deltas
  // (spf_graph_diff) and the overload bits choose the rows -- every row when
  // an overload bit flipped (the drained filter of every column the node
  // announces), else the rows spf_table_screen finds affected on the resident
  // SPF rows, closed by routeRefreshRowList -- the table's own graph is patched
  // (spf_graph_patch_metrics, spf_graph_set_transit), a new all-sources query
  // runs on it (the whole SPF: repairing only the affected rows is not done
  // here) and spf_route_table_refresh_rows recomputes the listed rows and
  // keeps the cells it replaced.  Adjacency labels are collected again.
  // Afterwards routes(), mplsRoutes(), countRoutes() describe the new
  // topology, changedSplit / delta / deltas give this call's delta with no
  // older table (MPLS: mplsEntry over the new cells against the same rule
  // over the previous cells and the previous adjacency labels), diff() works
  // with this table on either side, and applyPrefixChanges may follow.
  // A device failure after the graph was patched throws std::runtime_error and
  // leaves the table unusable (its graph, rows and cells no longer agree).
  // Returns the changed routes per node (unicast and node-label columns), id
  // order.
  // bgpColumns && bgpUseIgpMetric && bgpInPlace (with or without linksInPlace
  // and LFA): every BGP column of such a table is a selected column, whose
  // candidates, pair codes and loopback flags come from PrefixState alone;
  // reachability and the drain filter are read on the device.  The rows are
  // chosen as above and spf_route_table_refresh_rows_sel folds the selected
  // columns of the listed rows again in the same pass (previous igp words
  // kept: spf_route_table_fetch_cells_prev_igp); deltas() takes igp from the
  // pack's igp lane.  In a selected column best (its entry and loopback) and
  // igp are part of the route and a metric change moves best often: a changed
  // cell whose best alone moved -- the old and the new best candidate have
  // equal entries and equal loopbacks, and metric (non-LFA), links, link
  // metrics and igp all stayed -- is left out of the call's counts and delta,
  // as applyPrefixChanges does for kept selected columns (the changed cells of
  // columns that hold such a candidate pair are read back, now and previous).
  // linksInPlace: links of the table may also be down in `ls` or be back.  The
  // table's half-edges keep their CSR positions for its whole life; per node
  // they are matched to the half-edges of ls.engine() by Link identity (Link ==,
  // area, interface, v4 and v6 next-hop address from that node), within the
  // row and not by position.  A table half-edge without a partner is down; the
  // table keeps its Link object (previous cells may name it) until the link
  // returns, whose new object then replaces it.  Refused as above, before
  // anything is touched: an engine half-edge without a partner (a brand-new
  // link, or a returning one whose identity fields differ), node names or node
  // labels that differ, halves of one link that would end in different states,
  // a metric spf_graph_set_edges refuses (0, above 2^31 - 1, unpackable),
  // ls.engine().exact, borderNodes tables and the bgpColumns tables named
  // above.  The edge deltas are
  // spf_graph_diff of the table's up half-edges before the call and the
  // engine's CSR now; the rows are chosen as above with the tails of every
  // half-edge whose state or metric changed; ONE spf_graph_set_edges carries
  // every half-edge whose state changed together with the metric changes of
  // that call (spf_graph_patch_metrics when no state changed), then
  // spf_graph_set_transit, the new query, the refresh and the adjacency labels
  // as above.  A down half-edge never carries a link bit; diff() with such a
  // table on either side goes through the maps, where a down half-edge has no
  // counterpart.  A link that goes down can cut the smallest reachable
  // announcer of a prefix off: a cell whose `best` alone moved, between
  // announcers with equal PrefixEntries, is no route change and is left out of
  // the call's counts and delta (the changed cells of such columns are read
  // back, now and previous).
  std::vector<uint32_t> applyTopologyChanges(const LinkState& ls);
  // links of the table that are down now (linksInPlace)
  size_t downLinks() const { return downLinks_; }
  // device time of the last applyTopologyChanges' refresh kernel (its SPF: spfMs)
  float refreshMs() const { return refreshMs_; }
  // rows the last applyTopologyChanges listed
  size_t refreshRows() const { return refreshRows_; }
  // columns applyPrefixChanges can still give away
  size_t freeColumns() const { return freeList_.size(); }
  // free selected columns (spareSelectedColumns and freed ones)
  size_t freeSelectedColumns() const { return freeSelList_.size(); }
  // device time of the last applyPrefixChanges (bitmap clear + spf_route_patch_kernel)
  float patchMs() const { return patchMs_; }
  // BGP prefixes among them (bgpColumns), selected columns included
  size_t numBgpPrefixes() const { return nbgp_; }
  size_t numSelectedColumns() const { return nsel_; }

 private:
  // The cells of one table row, read through the accessors below: a whole
  // row (fetchRow), or a sparse view holding only the columns in `cols`
  // (deltas(): packed changed cells, spf_route_table_fetch_cells lists).
  struct Row {
    std::vector<uint32_t> metric, best;
    std::vector<uint64_t> links;
    std::vector<uint32_t> lmet; // LFA: per-link metrics [cols][deg]
    std::vector<uint32_t> igp;  // tables with selected columns: bestIgpMetric per cell
    size_t W = 0, deg = 0;
    bool sparse = false;
    std::vector<uint32_t> cols; // sparse: the columns held, ascending
    // storage index of column p
    size_t at(size_t p) const {
      if (!sparse) {
        return p;
      }
      auto it = std::lower_bound(cols.begin(), cols.end(), (uint32_t)p);
      if (it == cols.end() || *it != p) {
        throw std::logic_error("AllNodesRouteTable: column not in the sparse row view");
      }
      return (size_t)(it - cols.begin());
    }
    uint32_t metricOf(size_t p) const { return metric[at(p)]; }
    uint32_t bestOf(size_t p) const { return best[at(p)]; }
    const uint64_t* linksOf(size_t p) const { return links.data() + at(p) * W; }
    // metric of link j of cell p (LFA: its own, else the cell's)
    uint32_t linkMetric(size_t p, uint32_t j) const {
      const size_t s = at(p);
      return lmet.empty() ? metric[s] : lmet[s * deg + j];
    }
  };
  Row fetchRow(uint32_t i) const;
  // next hops of cell p of node i: make(link, metric) for every link of its mask
  template <class Make>
  std::unordered_set<thrift::NextHopThrift> cellNextHops(
      uint32_t i, const Row& r, size_t p, Make&& make) const;
  RibUnicastEntry materialise(const std::string& node, uint32_t i, const Row& r, size_t p) const;
  // the MPLS entry of `label` at node i: the node-label winner, else the
  // first adjacency label of that value
  std::optional<RibMplsEntry> mplsEntry(uint32_t i, const Row& r, int32_t label) const;
  struct AdjLabel;
  std::optional<RibMplsEntry> mplsEntryWith(
      uint32_t i, const Row& r, int32_t label, const std::vector<AdjLabel>& adj) const;
  // row i as it was before the last applyTopologyChanges (spf_route_table_fetch_cells_prev)
  Row fetchPrevRow(uint32_t i) const;
  std::optional<RibMplsEntry> nodeLabelEntry(uint32_t i, const Row& r, int32_t label) const;
  // The delta of one node from the last diff, shared by delta(node) and
  // deltas().  `cols` are the node's changed columns, `gone` its set bits of
  // the gone bitmap (indices into goneCols_).
  // MPLS candidates: labels of changed and gone label columns, both tables'
  // adjacency labels and, after a mapped diff, both node labels (ascending)
  std::vector<int32_t> labelCandidates(
      uint32_t i, const uint32_t* cols, size_t n, const uint32_t* gone, size_t ng) const;
  // unicast deletes of gone columns, then updates / deletes of changed ones
  // (`r` holds at least `cols`)
  void unicastDelta(
      uint32_t i, const Row& r, const uint32_t* cols, size_t n, const uint32_t* gone, size_t ng,
      DecisionRouteUpdate& u) const;
  // mplsEntry of every label here (row r) against `older_` (row o of its node
  // ia; SPF_MAP_NONE: every entry is new)
  void mplsDelta(
      uint32_t i, const Row& r, uint32_t ia, const Row& o, const std::vector<int32_t>& labels,
      DecisionRouteUpdate& u) const;

  struct Announcer {
    uint32_t id;
    thrift::PrefixEntry entry;
  };
  // a BGP column's host-side selection (bgpColumns)
  struct BgpSel {
    thrift::PrefixEntry bestEntry;
    std::string bestArea;
    std::optional<thrift::NextHopThrift> bestNexthop; // nullopt: no route anywhere
  };
  std::string area_;
  bool enableV4_;
  bool lfa_;
  std::vector<std::string> names_;
  std::unordered_map<std::string, uint32_t> ids_;
  std::vector<uint32_t> row_;                 // CSR row offsets of the snapshot
  // the rest of the CSR (applyTopologyChanges: layout check and edge deltas)
  std::vector<uint32_t> col_, rev_, linkId_;
  std::vector<uint64_t> metric_;
  uint32_t numLinks_{0};
  std::vector<std::shared_ptr<Link>> halfLink_; // half-edge -> Link
  std::vector<thrift::IpPrefix> prefixes_;
  std::vector<std::vector<Announcer>> announcers_;
  std::vector<std::optional<BgpSel>> bgp_; // per unicast slot (set: a BGP column)
  // a selected column (bgpUseIgpMetric): parallel to the column's announcers_
  // (= candidates, fold order)
  struct SelCol {
    std::vector<uint16_t> pair; // spf_route_select_desc::pair_codes of the column
    std::vector<std::optional<thrift::NextHopThrift>> via; // the candidate's one loopback via
  };
  std::vector<std::optional<SelCol>> sel_; // per unicast slot
  // The constructor's steps, in call order.  PrefixScan: what the constructor
  // was given and, per prefix of PrefixState in map order, what scanPrefix
  // found (keep: 0 not served, 1 Open/R, 2 BGP selected on the host, 3 a
  // selected column).
  struct PrefixScan {
    const LinkState* ls; // (null in applyPrefixChanges: overloaded_ answers instead)
    const PrefixState& ps;
    const std::unordered_set<std::string>* borderNodes;
    bool bgpColumns, bgpUseIgpMetric;
    std::vector<std::pair<const thrift::IpPrefix*, const thrift::PrefixEntries*>> items;
    std::vector<uint8_t> keep;
    std::vector<std::vector<Announcer>> anns;
    std::vector<std::optional<BgpSel>> sels;
    std::vector<std::optional<SelCol>> selCols;
    // BGP candidates: every in-graph announcer (the selection assumes each
    // is reachable from every node; dropUnreachableBgp checks)
    std::vector<std::vector<uint32_t>> bgpAll;
  };
  void scanPrefix(PrefixScan& s, size_t i) const;
  void dropUnreachableBgp(PrefixScan& s) const;
  // announcer id -> every node reaches it (one row fetch each, kept for
  // applyPrefixChanges: valid for the table's life since the rows are the
  // snapshot's; at most one entry per node).  Filled from the const
  // dropUnreachableBgp, which only the constructor and applyPrefixChanges
  // call: the object is not safe for concurrent use with applyPrefixChanges,
  // the const accessors do not touch it.
  mutable std::unordered_map<uint32_t, bool> reachesAll_;
  // annOff / ann: the announcer lists of every column, as the engine takes them
  void orderColumns(std::vector<uint32_t>& annOff, std::vector<uint32_t>& ann);
  void addNodeLabelColumns(
      const LinkState& ls, std::vector<uint32_t>& annOff, std::vector<uint32_t>& ann);
  void collectAdjLabels(const LinkState& ls);
  void createAndRunTable(const std::vector<uint32_t>& annOff, const std::vector<uint32_t>& ann);
  size_t nbgp_{0}, nsel_{0};
  size_t devSel_{0}; // selected columns of the device table (spare ones included)
  bool bgpColumns_{false}, bgpDryRun_{false}, bgpIgp_{false}, bgpInPlace_{false};
  // linksInPlace: down_[e] = half-edge e of the table's CSR is down (empty: none
  // ever was); col_ keeps every half-edge's head, down ones included
  bool linksInPlace_{false};
  std::vector<uint8_t> down_;
  size_t downLinks_{0};
  bool isDown(size_t e) const { return !down_.empty() && down_[e]; }
  std::vector<uint32_t> applyLinkChanges(const LinkState& ls);
  // applyTopologyChanges, both forms: the refusals by how the table was built
  // (throws std::invalid_argument), the refresh call by the kind of device
  // table, and -- after the refresh, suppress_ assigned -- the selected
  // columns' changed cells whose `best` alone moved onto an equal candidate
  // (same entry, same loopback; metric, links, link metrics, igp stayed): read
  // back now and previous, added to suppress_ and taken out of counts
  void refuseTopologyChanges(const char* who) const;
  void refreshListedRows(spf_query* q, bool all, const std::vector<uint32_t>& rows,
                         std::vector<uint32_t>& counts);
  void suppressSelectedBest(std::vector<uint32_t>& counts);
  std::vector<uint8_t> overloaded_; // per node id, from the snapshot (scanPrefix without LinkState)
  // 0 Open/R, 1 BGP selected on the host, 2 a selected column -- by what the
  // column serves (a free column is an Open/R one)
  int columnKind(size_t c) const {
    if (!isUni(c) || slotOf(c) >= sel_.size()) {
      return 0;
    }
    return sel_[slotOf(c)] ? 2 : bgp_[slotOf(c)] ? 1 : 0;
  }
  // the device column is a selected one (fixed at creation)
  bool selectedColumn(size_t c) const {
    return c < prefixes_.size() ? ctorSel_[c] != 0 : c >= spareBase() + spare_;
  }
  std::vector<uint8_t> ctorSel_; // per constructor column: created as a selected column
  const SelCol& selAt(size_t c) const { return *sel_[slotOf(c)]; }
  const BgpSel& bgpAt(size_t c) const { return *bgp_[slotOf(c)]; }
  // Column layout: [0, prefixes_.size()) the constructor's unicast columns,
  // then owners_.size() node-label columns, then spare_ spare columns, then
  // spareSel_ spare selected columns.  A unicast column has a slot: its index,
  // or prefixes_.size() + j for spare column j (of either kind).  free_[slot]: the column serves no prefix (its prefix entry is
  // the last one it served, read by the delete of that call's delta).
  size_t spare_{0}, spareSel_{0};
  std::vector<uint32_t> freeSelList_; // free selected columns, taken from the back
  std::vector<thrift::IpPrefix> sparePrefix_;
  std::vector<std::vector<Announcer>> spareAnn_;
  std::vector<uint8_t> free_;
  std::vector<uint32_t> freeList_; // free columns, taken from the back
  bool holes_{false};              // spare or freed columns exist: served_ is prefixes()
  std::vector<thrift::IpPrefix> served_;
  std::unordered_map<thrift::IpPrefix, uint32_t> colOfPrefix_; // served prefix -> column
  bool hasBorder_{false};
  bool patchDelta_{false}; // the last delta is applyPrefixChanges' (older_ is null)
  // the last delta is applyTopologyChanges' (older_ is null): the older side
  // is this table's previous cells and prevAdjLabels_
  bool topoDelta_{false};
  float refreshMs_{0};
  size_t refreshRows_{0};
  float patchMs_{0};
  // per node: columns of the last applyPrefixChanges or applyTopologyChanges
  // whose cell changed in `best` alone, between announcers with equal
  // PrefixEntries (no route change; a link that goes down can cut the best
  // announcer of an anycast prefix off)
  std::vector<std::vector<uint32_t>> suppress_;
  bool suppressed(uint32_t i, uint32_t c) const {
    return (patchDelta_ || topoDelta_) &&
        std::binary_search(suppress_[i].begin(), suppress_[i].end(), c);
  }
  size_t numCols() const { return prefixes_.size() + owners_.size() + spare_ + spareSel_; }
  size_t spareBase() const { return prefixes_.size() + owners_.size(); }
  bool isUni(size_t c) const { return c < prefixes_.size() || c >= spareBase(); }
  size_t slotOf(size_t c) const { return c < prefixes_.size() ? c : c - owners_.size(); }
  bool isFree(size_t c) const { return !free_.empty() && free_[slotOf(c)]; }
  const thrift::IpPrefix& prefixAt(size_t c) const {
    return c < prefixes_.size() ? prefixes_[c] : sparePrefix_[c - spareBase()];
  }
  const std::vector<Announcer>& annsAt(size_t c) const {
    return c < prefixes_.size() ? announcers_[c] : spareAnn_[c - spareBase()];
  }
  void rebuildServed();
  static bool sameSelection(const BgpSel& a, const BgpSel& b);
  // node-label columns: column prefixes_.size() + k is owners_[k]
  struct LabelOwner {
    int32_t label;
    uint32_t id;
  };
  std::vector<LabelOwner> owners_;
  std::map<int32_t, std::vector<uint32_t>> labelCols_; // label -> owner columns by name
  // adjacency labels of every node, linksFromNode order (values copied)
  struct AdjLabel {
    int32_t label;
    thrift::BinaryAddress nhV6;
    std::string iface;
    int32_t metric;
    std::string area;
  };
  std::vector<std::vector<AdjLabel>> adjLabels_;
  std::vector<std::vector<AdjLabel>> prevAdjLabels_; // before the last applyTopologyChanges
  std::vector<int32_t> nodeLabel_; // per node id: its valid node label, else 0
  const AllNodesRouteTable* older_{nullptr};
  // the last diff(): older row of every node (SPF_MAP_NONE: none) and, when
  // it went through the maps, the older columns with no counterpart here
  bool mapped_{false};
  std::vector<uint32_t> rowOf_;
  std::vector<uint32_t> goneCols_;
  // parallel to goneCols_: the newer column of the same prefix when the
  // column changed its kind, else SPF_MAP_NONE
  std::vector<uint32_t> goneNew_;
  float diffCallMs_{0};
  mutable DeltasStats lastDeltas_;
  std::vector<uint32_t> diffMapped(const AllNodesRouteTable& older);
  // engine handles, declared so that destruction runs table, query, graph
  struct GraphDeleter {
    void operator()(spf_graph* g) const { spf_graph_destroy(g); }
  };
  struct QueryDeleter {
    void operator()(spf_query* q) const { spf_query_destroy(q); }
  };
  struct TableDeleter {
    void operator()(spf_route_table* t) const { spf_route_table_destroy(t); }
  };
  std::unique_ptr<spf_graph, GraphDeleter> graph_;
  std::unique_ptr<spf_query, QueryDeleter> query_;
  std::unique_ptr<spf_route_table, TableDeleter> table_;
  float spfMs_{0}, routeMs_{0}, selectMs_{0};
  bool diffed_{false};
};

// Every node's COMPLETE RouteDb over all areas (SURVEY §8(f) row 1 beyond
// one area and IGP prefixes): routeDb(node) == SpfSolver::buildRouteDb(node)
// (Decision.cpp:291-542) for any configuration -- multi-area, BGP,
// SR-MPLS / KSP2.  Device share: one AllNodesRouteTable per area (all-sources
// SPF + spf_route_table_kernel) serves the IP / SP_ECMP Open/R prefixes of
// the area's interior nodes (single area: every node, MPLS node labels
// included); the host share is SpfSolver::buildRouteDbPartial over the
// same LinkStates for what the kernel does not restate: border nodes (in two
// or more areas: cross-area ECMP and drain rules), BGP prefixes the tables
// do not take (metric-vector best path, Decision.cpp:714-866; with
// bgpUseIgpMetric all of them unless bgpIgpOnDevice makes them selected
// columns of the area's table), SR-MPLS prefixes, prefixes a border node
// announces, and the multi-area MPLS routes.  With
// prefetchAll, every area's all-sources SPF views are computed in one
// device batch up front, so the host share runs no SPF per node.
class AllAreasRouteTable {
 public:
  AllAreasRouteTable(
      const std::unordered_map<std::string, LinkState>& areas, const PrefixState& ps,
      bool enableV4 = true, bool computeLfa = false, bool bgpDryRun = false,
      bool bgpUseIgpMetric = false, bool prefetchAll = true, bool bgpIgpOnDevice = false);
  ~AllAreasRouteTable();
  // nullopt iff `node` is in no area (Decision.cpp:296-302)
  std::optional<DecisionRouteDb> routeDb(const std::string& node) const;
  // routes of the last routeDb() call that came from a device table / the host
  size_t lastTableRoutes() const { return lastTable_; }
  size_t lastHostRoutes() const { return lastHost_; }
  bool isBorder(const std::string& node) const { return border_.count(node) > 0; }
  // the device table of `area` (null: unknown area, or one left to the host),
  // so that a holder of two all-areas tables can diff the device share per
  // area; a whole all-areas delta with border nodes and the host share is
  // not built here
  const AllNodesRouteTable* areaTable(const std::string& area) const;
  // (diff() keeps its bitmaps in the newer table: the holder of a non-const
  // all-areas table diffs through this one)
  AllNodesRouteTable* areaTable(const std::string& area) {
    return const_cast<AllNodesRouteTable*>(std::as_const(*this).areaTable(area));
  }
  size_t numTables() const { return tables_.size(); }
  // BGP prefixes the device tables serve (round 6; AllNodesRouteTable
  // bgpColumns)
  size_t numBgpDevicePrefixes() const {
    size_t n = 0;
    for (const auto& [_, t] : tables_) {
      n += t->numBgpPrefixes();
    }
    return n;
  }
  // device time of the tables' route / selection kernels, summed over areas
  float routeMs() const {
    float ms = 0;
    for (const auto& [_, t] : tables_) {
      ms += t->routeMs();
    }
    return ms;
  }
  float selectMs() const {
    float ms = 0;
    for (const auto& [_, t] : tables_) {
      ms += t->selectMs();
    }
    return ms;
  }

 private:
  const std::unordered_map<std::string, LinkState>& areas_;
  const PrefixState& ps_;
  bool enableV4_, lfa_, bgpDryRun_, bgpIgp_;
  std::unordered_set<std::string> border_;
  std::unordered_map<std::string, std::string> home_; // interior node -> its area
  std::map<std::string, std::unique_ptr<AllNodesRouteTable>> tables_;
  std::map<std::string, std::unordered_set<thrift::IpPrefix>> served_;
  std::map<std::string, bool> rest_; // area -> some prefix is left to the host
  mutable size_t lastTable_{0}, lastHost_{0};
};

} // namespace openr
