// RouteTable.cpp — AllNodesRouteTable (see RouteTable.h).

#include "RouteTable.h"

#include <algorithm>
#include <chrono>
#include <set>
#include <stdexcept>

#include "Engine.h"
#include "Parallel.h"
#include "Util.h"

namespace openr {

namespace {
int64_t usSince(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration_cast<std::chrono::microseconds>(
             std::chrono::steady_clock::now() - t0)
      .count();
}

[[noreturn]] void tableFailure(const char* what, int status) {
  throw std::runtime_error(
      std::string("openr_spf: ") + what + ": " + spf_error_string(status) + " (" +
      spf_last_error_detail() + ")");
}

// f(index) for every set bit of words[0 .. n), ascending
template <class F>
void forEachSetBit(const uint64_t* words, size_t n, F&& f) {
  for (size_t k = 0; k < n; ++k) {
    for (uint64_t m = words[k]; m; m &= m - 1) {
      f(k * 64 + (size_t)__builtin_ctzll(m));
    }
  }
}
} // namespace

// eligibility and announcers of prefix i (Decision.cpp:313-412 restricted to
// selectEcmpOpenr, and with bgpColumns selectEcmpBgp): read-only PrefixState
// lookups, one prefix per call on the host pool
void AllNodesRouteTable::scanPrefix(PrefixScan& s, size_t i) const {
  const PrefixState& ps = s.ps;
  const auto* borderNodes = s.borderNodes;
  const bool bgpColumns = s.bgpColumns, bgpUseIgpMetric = s.bgpUseIgpMetric;
  auto& keep = s.keep;
  auto& anns = s.anns;
  auto& bgpAll = s.bgpAll;
  auto& sels = s.sels;
  auto& selCols = s.selCols;
  const auto& prefix = *s.items[i].first;
  const auto& entries = *s.items[i].second;
  bool otherArea = false, bgp = false, nonBgp = false, missingMv = false, inArea = false,
       borderAnn = false;
  for (const auto& [node, byArea] : entries) {
    for (const auto& [area, entry] : byArea) {
      otherArea |= area != area_;
      inArea |= area == area_;
      borderAnn |= area == area_ && borderNodes && borderNodes->count(node);
      const bool isBgp = entry.type == thrift::PrefixType::BGP;
      bgp |= isBgp;
      nonBgp |= !isBgp;
      missingMv |= isBgp && !entry.mv.has_value();
    }
  }
  if ((bgp && !bgpColumns) || (bgp && (nonBgp || missingMv)) || entries.empty() ||
      (otherArea && !borderNodes) || !inArea || borderAnn) {
    return;
  }
  if (prefix.prefixAddress.addr.size() == 4 && !enableV4_) {
    return;
  }
  if (getPrefixForwardingType(entries) != thrift::PrefixForwardingType::IP ||
      getPrefixForwardingAlgorithm(entries) != thrift::PrefixForwardingAlgorithm::SP_ECMP) {
    return;
  }
  if (!bgp) {
    for (const auto& [node, byArea] : entries) {
      auto it = ids_.find(node);
      auto ea = byArea.find(area_);
      if (it == ids_.end() || ea == byArea.end()) {
        continue; // not in the graph / announced in another area: never reachable
      }
      anns[i].push_back(Announcer{it->second, ea->second});
    }
    keep[i] = 1;
    return;
  }
  if (otherArea) {
    return; // (interior-node tables of several areas: BGP stays on the host)
  }
  namespace mvu = MetricVectorUtils;
  if (bgpUseIgpMetric) {
    // a selected column: the fold runs per node on the device
    // (spf_route_select_kernel).  Candidates = in-graph announcers in
    // fold order, without those that advertise OPENR_IGP_COST
    // (Decision.cpp:735-744: skipped before bestIgpMetric sees them)
    SelCol sc;
    std::vector<const thrift::MetricVector*> mvs;
    const bool isV4 = prefix.prefixAddress.addr.size() == 4;
    for (const auto& [node, byArea] : entries) {
      for (const auto& [area, entry] : byArea) {
        auto it = ids_.find(node);
        if (it == ids_.end()) {
          continue; // not in the graph: unreachable from every node
        }
        const thrift::MetricVector& mv = entry.mv.value();
        if (mvu::getMetricEntityByType(mv, mvu::kOpenrIgpCostType)) {
          continue;
        }
        for (const auto& me : mv.metrics) {
          if (me.priority == mvu::kOpenrIgpCostPriority) {
            return; // std::sort leaves its order against the IGP entity open: host
          }
        }
        anns[i].push_back(Announcer{it->second, entry});
        mvs.push_back(&mv);
        auto vias = ps.getLoopbackVias({node}, isV4, std::nullopt);
        sc.via.push_back(vias.size() == 1 ? std::optional<thrift::NextHopThrift>(vias[0])
                                          : std::nullopt);
      }
    }
    if (mvs.size() > 32) {
      anns[i].clear();
      return; // the winners word has 32 bits: host
    }
    for (size_t c = 1; c < mvs.size(); ++c) {
      for (size_t b = 0; b < c; ++b) {
        const auto codes = mvu::bgpIgpPairCodes(*mvs[c], *mvs[b]);
        sc.pair.push_back((uint16_t)((unsigned)codes[0] | ((unsigned)codes[1] << 3) |
                                     ((unsigned)codes[2] << 6)));
      }
    }
    selCols[i] = std::move(sc);
    keep[i] = 3;
    return;
  }
  // runBestPathSelectionBgp (Decision.cpp:714-803) without the IGP
  // cost, every in-graph announcer reachable: entries in map order
  std::optional<thrift::MetricVector> bestVector;
  std::set<std::string> winners;
  std::string bestNode, bestArea;
  for (const auto& [node, byArea] : entries) {
    for (const auto& [area, entry] : byArea) {
      auto it = ids_.find(node);
      if (it == ids_.end()) {
        continue; // not in the graph: unreachable from every node
      }
      bgpAll[i].push_back(it->second);
      const thrift::MetricVector& mvIn = entry.mv.value();
      if (mvu::getMetricEntityByType(mvIn, mvu::kOpenrIgpCostType)) {
        continue;
      }
      thrift::MetricVector mv = mvIn;
      mvu::CompareResult cmp = mvu::CompareResult::WINNER;
      if (bestVector) {
        cmp = mvu::compareMetricVectors(mv, *bestVector);
      }
      switch (cmp) {
      case mvu::CompareResult::WINNER:
        winners.clear();
        [[fallthrough]];
      case mvu::CompareResult::TIE_WINNER:
        bestVector = std::move(mv);
        bestNode = node;
        bestArea = area;
        [[fallthrough]];
      case mvu::CompareResult::TIE_LOOSER:
        winners.insert(node);
        break;
      case mvu::CompareResult::TIE:
      case mvu::CompareResult::ERROR:
        // cannot order: no route at any node
        sels[i] = BgpSel{};
        keep[i] = 2;
        return;
      default:
        break;
      }
    }
  }
  BgpSel sel;
  if (!winners.empty()) {
    // maybeFilterDrainedNodes (Decision.cpp:651-666)
    std::set<std::string> undrained;
    for (const auto& w : winners) {
      if (!(s.ls ? s.ls->isNodeOverloaded(w) : overloaded_[ids_.at(w)] != 0)) {
        undrained.insert(w);
      }
    }
    const auto& use = undrained.empty() ? winners : undrained;
    auto vias = ps.getLoopbackVias({bestNode}, prefix.prefixAddress.addr.size() == 4,
                                   std::nullopt);
    if (vias.size() == 1) {
      sel.bestEntry = entries.at(bestNode).at(bestArea);
      sel.bestArea = bestArea;
      sel.bestNexthop = vias.at(0);
      for (const auto& w : use) {
        anns[i].push_back(Announcer{ids_.at(w), entries.at(w).at(area_)});
      }
    }
  }
  sels[i] = std::move(sel);
  keep[i] = 2;
}

// BGP columns need every in-graph announcer reachable from every node:
// reachability is symmetric here (links are up in both directions and a
// path's interior nodes are the same either way), so the announcer's
// own row answers for every node
void AllNodesRouteTable::dropUnreachableBgp(PrefixScan& s) const {
  const uint32_t V = (uint32_t)names_.size();
  auto& reachesAll = reachesAll_; // (the rows are the snapshot's: an answer holds for the table's life)
  std::vector<uint32_t> rowBuf(V);
  for (size_t i = 0; i < s.items.size(); ++i) {
    if (s.keep[i] != 2) {
      continue;
    }
    for (const uint32_t a : s.bgpAll[i]) {
      auto it = reachesAll.find(a);
      if (it == reachesAll.end()) {
        if (int st = spf_query_fetch_rows(query_.get(), a, 1, rowBuf.data(), (size_t)V * 4, 0);
            st != SPF_OK) {
          tableFailure("spf_query_fetch_rows", st);
        }
        const bool all = std::all_of(rowBuf.begin(), rowBuf.end(),
                                     [](uint32_t x) { return x != 0xFFFFFFFFu; });
        it = reachesAll.emplace(a, all).first;
      }
      if (!it->second) {
        s.keep[i] = 0; // some node does not reach this announcer: the host path
        break;
      }
    }
  }
}

// prefix order: by first announcer id, so neighbouring lanes of the
// kernel read neighbouring distance / next-hop mask words of a row
void AllNodesRouteTable::orderColumns(std::vector<uint32_t>& annOff, std::vector<uint32_t>& ann) {
  std::vector<uint32_t> order(prefixes_.size());
  for (uint32_t i = 0; i < order.size(); ++i) {
    order[i] = i;
  }
  auto key = [&](uint32_t i) {
    return announcers_[i].empty() ? 0xFFFFFFFFu : announcers_[i][0].id;
  };
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t x, uint32_t y) { return key(x) < key(y); });
  std::vector<thrift::IpPrefix> px;
  std::vector<std::vector<Announcer>> ax;
  std::vector<std::optional<BgpSel>> bx;
  std::vector<std::optional<SelCol>> sx;
  sx.reserve(order.size());
  px.reserve(order.size());
  ax.reserve(order.size());
  bx.reserve(order.size());
  for (uint32_t i : order) {
    px.push_back(std::move(prefixes_[i]));
    ax.push_back(std::move(announcers_[i]));
    bx.push_back(std::move(bgp_[i]));
    sx.push_back(std::move(sel_[i]));
  }
  sel_ = std::move(sx);
  prefixes_ = std::move(px);
  announcers_ = std::move(ax);
  bgp_ = std::move(bx);
  for (const auto& as : announcers_) {
    for (const auto& a : as) {
      ann.push_back(a.id);
    }
    annOff.push_back((uint32_t)ann.size());
  }
}

// node-label columns (Decision.cpp:415-481): one pseudo-prefix per (valid
// label, owner in the graph), owners of a label by name; the cell of node
// s is getNextHopsWithMetric(s, {owner}) with LFA off
void AllNodesRouteTable::addNodeLabelColumns(
    const LinkState& ls, std::vector<uint32_t>& annOff, std::vector<uint32_t>& ann) {
  // (label, owner id) sorted: labels ascending, owners by name (ids are
  // name ranks) -- the order of a label -> sorted names map, without one
  std::vector<std::pair<int32_t, uint32_t>> lab;
  lab.reserve(names_.size());
  nodeLabel_.assign(names_.size(), 0);
  for (const auto& [node, db] : ls.getAdjacencyDatabases()) {
    if (db.nodeLabel == 0 || !isMplsLabelValid(db.nodeLabel)) {
      continue;
    }
    auto it = ids_.find(node);
    if (it != ids_.end()) {
      lab.emplace_back(db.nodeLabel, it->second);
      nodeLabel_[it->second] = db.nodeLabel;
    }
  }
  std::sort(lab.begin(), lab.end());
  for (size_t i = 0; i < lab.size();) {
    auto& cols =
        labelCols_.emplace_hint(labelCols_.end(), lab[i].first, std::vector<uint32_t>{})->second;
    size_t j = i;
    for (; j < lab.size() && lab[j].first == lab[i].first; ++j) {
      cols.push_back((uint32_t)(prefixes_.size() + owners_.size()));
      owners_.push_back(LabelOwner{lab[j].first, lab[j].second});
      ann.push_back(lab[j].second);
      annOff.push_back((uint32_t)ann.size());
    }
    i = j;
  }
}

// adjacency labels of every node (Decision.cpp:511-534), values copied
// (independent per node: read-only LinkState lookups on the host pool)
void AllNodesRouteTable::collectAdjLabels(const LinkState& ls) {
  adjLabels_.resize(names_.size());
  parallelFor(names_.size(), hostThreads(names_.size(), 256), [&](size_t i, unsigned) {
    for (const auto& link : ls.linksFromNode(names_[i])) {
      const int32_t label = link->getAdjLabelFromNode(names_[i]);
      if (label == 0 || !isMplsLabelValid(label)) {
        continue;
      }
      adjLabels_[i].push_back(AdjLabel{
          label, link->getNhV6FromNode(names_[i]), link->getIfaceFromNode(names_[i]),
          (int32_t)link->getMetricFromNode(names_[i]), link->getArea()});
    }
  }, 64);
}

// selected columns (pair tables and loopback bits parallel to ann), then the
// engine's table over every column, created and run
void AllNodesRouteTable::createAndRunTable(
    const std::vector<uint32_t>& annOff, const std::vector<uint32_t>& ann) {
  auto tp = std::chrono::steady_clock::now();
  std::vector<uint32_t> selColumns;
  std::vector<uint64_t> pairOff{0};
  std::vector<uint16_t> pairCodes;
  std::vector<uint8_t> candFlags(ann.size(), 0);
  for (size_t p = 0; p < prefixes_.size(); ++p) {
    if (!sel_[p]) {
      continue;
    }
    selColumns.push_back((uint32_t)p);
    pairCodes.insert(pairCodes.end(), sel_[p]->pair.begin(), sel_[p]->pair.end());
    pairOff.push_back(pairCodes.size());
    for (size_t c = 0; c < sel_[p]->via.size(); ++c) {
      candFlags[annOff[p] + c] = sel_[p]->via[c] ? 1 : 0;
    }
  }
  nsel_ = selColumns.size();
  ctorSel_.assign(prefixes_.size(), 0);
  for (const uint32_t p : selColumns) {
    ctorSel_[p] = 1;
  }
  for (size_t j = 0; j < spareSel_; ++j) { // spare selected columns: no candidates, no pair codes
    selColumns.push_back((uint32_t)(spareBase() + spare_ + j));
    pairOff.push_back(pairCodes.size());
  }
  devSel_ = selColumns.size();
  spf_route_select_desc sd{};
  sd.num_selected = (uint32_t)selColumns.size();
  sd.columns = selColumns.data();
  sd.pair_offsets = pairOff.data();
  sd.pair_codes = pairCodes.data();
  sd.cand_flags = candFlags.data();
  int s = SPF_OK;
  spf_route_table* table = nullptr;
  if ((s = spf_route_table_create_sel(
           query_.get(), (uint32_t)numCols(), annOff.data(),
           ann.empty() ? nullptr : ann.data(), lfa_ ? SPF_RT_LFA : 0u, devSel_ ? &sd : nullptr,
           &table)) != SPF_OK) {
    tableFailure("spf_route_table_create", s);
  }
  table_.reset(table);
  if (lfa_) {
    // every LFA next hop carries its own metric (compared link by link): the
    // cell's metric word, the shortest distance, is no part of a route, and a
    // drained neighbour can raise it while the route stays the same
    if ((s = spf_route_table_diff_routes(table_.get(), 1)) != SPF_OK) {
      tableFailure("spf_route_table_diff_routes", s);
    }
  }
  Counters::add("decision.route_table_create_us", usSince(tp));
  tp = std::chrono::steady_clock::now();
  if ((s = spf_route_table_run(table_.get())) != SPF_OK) {
    tableFailure("spf_route_table_run", s);
  }
  if ((s = spf_query_elapsed_ms(query_.get(), &spfMs_)) != SPF_OK ||
      (s = spf_route_table_elapsed_ms(table_.get(), &routeMs_)) != SPF_OK ||
      (s = spf_route_table_select_elapsed_ms(table_.get(), &selectMs_)) != SPF_OK) {
    tableFailure("elapsed", s);
  }
  Counters::add("decision.route_table_run_us", usSince(tp));
}

AllNodesRouteTable::AllNodesRouteTable(
    const LinkState& ls, const PrefixState& ps, bool enableV4, bool computeLfa,
    const std::unordered_set<std::string>* borderNodes, bool bgpColumns, bool bgpDryRun,
    bool bgpUseIgpMetric, size_t spareColumns, bool bgpInPlace, size_t spareSelectedColumns,
    bool linksInPlace)
    : area_(ls.getArea()),
      enableV4_(enableV4),
      lfa_(computeLfa),
      bgpColumns_(bgpColumns),
      bgpDryRun_(bgpDryRun),
      bgpIgp_(bgpUseIgpMetric),
      bgpInPlace_(bgpInPlace),
      linksInPlace_(linksInPlace),
      spare_(spareColumns),
      spareSel_(bgpColumns && bgpUseIgpMetric ? spareSelectedColumns : 0),
      hasBorder_(borderNodes != nullptr) {
  auto tp = std::chrono::steady_clock::now();
  LinkState::Engine& eng = ls.engine();
  Counters::add("decision.route_table_engine_us", usSince(tp));
  tp = std::chrono::steady_clock::now();
  if (eng.exact) {
    throw std::invalid_argument(
        "AllNodesRouteTable: metric 0 / 64-bit sums need the exact kernel");
  }
  names_ = eng.names;
  ids_ = eng.ids;
  overloaded_.assign(eng.overloaded.begin(), eng.overloaded.end());
  row_ = eng.row;
  col_ = eng.col;
  rev_ = eng.rev;
  linkId_ = eng.linkId;
  metric_ = eng.metric;
  numLinks_ = (uint32_t)eng.links.size();
  halfLink_.resize(eng.col.size());
  for (size_t e = 0; e < eng.col.size(); ++e) {
    halfLink_[e] = eng.links[eng.linkId[e]];
  }
  // own snapshot of the device graph (the table outlives LinkState changes)
  // and the all-sources query, first: BGP columns check reachability on it
  spf_graph_desc d{};
  d.num_nodes = (uint32_t)eng.names.size();
  d.num_edges = (uint32_t)eng.col.size();
  d.row_ptr = eng.row.data();
  d.col = eng.col.data();
  d.metric = eng.metric.data();
  d.link_id = eng.linkId.data();
  d.rev = eng.rev.data();
  d.node_overloaded = eng.overloaded.data();
  d.num_links = (uint32_t)eng.links.size();
  d.device = getSpfDevice();
  // (a failure below throws: the handles created so far are members already)
  spf_graph* graph = nullptr;
  if (int s = spf_graph_create(&d, &graph); s != SPF_OK) {
    tableFailure("spf_graph_create", s);
  }
  graph_.reset(graph);
  Counters::add("decision.route_table_graph_us", usSince(tp));
  tp = std::chrono::steady_clock::now();
  std::vector<uint32_t> src(d.num_nodes);
  for (uint32_t i = 0; i < d.num_nodes; ++i) {
    src[i] = i;
  }
  spf_query_desc qd{};
  qd.num_queries = d.num_nodes;
  qd.sources = src.data();
  qd.flags = SPF_F_NEXTHOPS;
  int s = SPF_OK;
  spf_query* query = nullptr;
  if ((s = spf_query_create(graph_.get(), &qd, &query)) != SPF_OK) {
    tableFailure("spf_query_create", s);
  }
  query_.reset(query);
  if ((s = spf_query_run(query_.get())) != SPF_OK) {
    tableFailure("spf_query_run", s);
  }
  Counters::add("decision.route_table_query_us", usSince(tp));
  tp = std::chrono::steady_clock::now();
  std::vector<uint32_t> annOff{0}, ann;
  {
    // eligible prefixes with their announcers, kept in the map's iteration order
    PrefixScan scan{&ls, ps, borderNodes, bgpColumns, bgpUseIgpMetric};
    scan.items.reserve(ps.prefixes().size());
    for (const auto& [prefix, entries] : ps.prefixes()) {
      scan.items.emplace_back(&prefix, &entries);
    }
    const size_t n = scan.items.size();
    scan.keep.assign(n, 0);
    scan.anns.resize(n);
    scan.sels.resize(n);
    scan.selCols.resize(n);
    scan.bgpAll.resize(n);
    parallelFor(n, hostThreads(n, 256), [&](size_t i, unsigned) { scanPrefix(scan, i); }, 64);
    dropUnreachableBgp(scan);
    for (size_t i = 0; i < n; ++i) {
      if (scan.keep[i]) {
        prefixes_.push_back(*scan.items[i].first);
        announcers_.push_back(std::move(scan.anns[i]));
        bgp_.push_back(scan.keep[i] == 2 ? std::move(scan.sels[i]) : std::nullopt);
        sel_.push_back(std::move(scan.selCols[i]));
        nbgp_ += scan.keep[i] >= 2;
      }
    }
  }
  orderColumns(annOff, ann);
  Counters::add("decision.route_table_prefixes_us", usSince(tp));
  addNodeLabelColumns(ls, annOff, ann);
  Counters::add("decision.route_table_labels_us", usSince(tp));
  if (spare_ + spareSel_) {
    // spare columns: empty lists after the label columns, all free; the spare
    // selected columns after them
    annOff.insert(annOff.end(), spare_ + spareSel_, (uint32_t)ann.size());
    sparePrefix_.resize(spare_ + spareSel_);
    spareAnn_.resize(spare_ + spareSel_);
    bgp_.resize(prefixes_.size() + spare_ + spareSel_);
    sel_.resize(prefixes_.size() + spare_ + spareSel_);
    free_.assign(prefixes_.size() + spare_ + spareSel_, 0);
    for (size_t j = spare_ + spareSel_; j-- > 0;) {
      free_[prefixes_.size() + j] = 1;
      // (taken from the back: ascending)
      (j < spare_ ? freeList_ : freeSelList_).push_back((uint32_t)(spareBase() + j));
    }
    rebuildServed();
  }
  collectAdjLabels(ls);
  Counters::add("decision.route_table_host_us", usSince(tp)); // (from the same start)
  createAndRunTable(annOff, ann);
  Counters::add("decision.route_table_builds", 1);
}

AllNodesRouteTable::~AllNodesRouteTable() {
  const auto tp = std::chrono::steady_clock::now();
  table_.reset();
  query_.reset();
  graph_.reset();
  Counters::add("decision.route_table_destroy_us", usSince(tp));
}

uint64_t AllNodesRouteTable::countRoutes() const {
  uint64_t n = 0;
  const size_t C = numCols();
  std::vector<uint32_t> metric(C), best(C);
  std::vector<uint64_t> links;
  for (uint32_t i = 0; i < names_.size(); ++i) {
    const int w = spf_route_table_link_words(table_.get(), i);
    links.resize(std::max<size_t>(1, C * (size_t)std::max(w, 0)));
    if (int s = spf_route_table_fetch(table_.get(), i, metric.data(), best.data(), links.data());
        s != SPF_OK) {
      tableFailure("spf_route_table_fetch", s);
    }
    for (size_t p = 0; p < C; ++p) {
      n += isUni(p) && metric[p] != 0xFFFFFFFFu;
    }
  }
  return n;
}

AllNodesRouteTable::Row AllNodesRouteTable::fetchRow(uint32_t i) const {
  Row r;
  const int w = spf_route_table_link_words(table_.get(), i);
  if (w < 0) {
    tableFailure("spf_route_table_link_words", w);
  }
  const size_t P = numCols();
  r.W = (size_t)w;
  r.metric.resize(P);
  r.best.resize(P);
  r.links.resize(std::max<size_t>(1, P * r.W));
  if (devSel_) {
    r.igp.resize(P);
    std::vector<uint32_t> winners(P);
    if (int s = spf_route_table_fetch_sel(table_.get(), i, r.metric.data(), r.best.data(),
                                          r.links.data(), r.igp.data(), winners.data());
        s != SPF_OK) {
      tableFailure("spf_route_table_fetch_sel", s);
    }
  } else if (int s = spf_route_table_fetch(table_.get(), i, r.metric.data(), r.best.data(),
                                           r.links.data());
             s != SPF_OK) {
    tableFailure("spf_route_table_fetch", s);
  }
  if (lfa_) {
    r.deg = row_[i + 1] - row_[i];
    r.lmet.resize(std::max<size_t>(1, P * r.deg));
    if (int s = spf_route_table_fetch_link_metrics(table_.get(), i, r.lmet.data()); s != SPF_OK) {
      tableFailure("spf_route_table_fetch_link_metrics", s);
    }
  }
  return r;
}

template <class Make>
std::unordered_set<thrift::NextHopThrift> AllNodesRouteTable::cellNextHops(
    uint32_t i, const Row& r, size_t p, Make&& make) const {
  std::unordered_set<thrift::NextHopThrift> nhs;
  const uint32_t e0 = row_[i];
  forEachSetBit(r.W ? r.linksOf(p) : nullptr, r.W, [&](size_t j) {
    nhs.insert(make(*halfLink_[e0 + j], (int32_t)r.linkMetric(p, (uint32_t)j)));
  });
  return nhs;
}

RibUnicastEntry AllNodesRouteTable::materialise(
    const std::string& node, uint32_t i, const Row& r, size_t p) const {
  const bool isV4 = prefixAt(p).prefixAddress.addr.size() == 4;
  auto nhs = cellNextHops(i, r, p, [&](const Link& l, int32_t metric) {
    return createNextHop(
        isV4 ? l.getNhV4FromNode(node) : l.getNhV6FromNode(node), l.getIfaceFromNode(node),
        metric, std::nullopt, false, l.getArea());
  });
  if (columnKind(p) == 2) {
    // selectEcmpBgp (Decision.cpp:805-866) per node: the cell's best
    // candidate, its loopback with the cell's igp as metric
    // (PrefixState.cpp:111-126)
    const SelCol& sc = selAt(p);
    const auto& cands = annsAt(p);
    for (size_t c = 0; c < cands.size(); ++c) {
      if (cands[c].id == r.bestOf(p) && sc.via[c]) {
        thrift::NextHopThrift via = *sc.via[c];
        via.metric = (int32_t)r.igp[r.at(p)];
        return RibUnicastEntry(prefixAt(p), std::move(nhs), cands[c].entry, area_, bgpDryRun_,
                               via);
      }
    }
    throw std::logic_error("AllNodesRouteTable: best candidate not in the selected column");
  }
  if (columnKind(p) == 1) {
    // selectEcmpBgp (Decision.cpp:805-866): the host-side selection's best
    const BgpSel& b = bgpAt(p);
    return RibUnicastEntry(prefixAt(p), std::move(nhs), b.bestEntry, b.bestArea, bgpDryRun_,
                           b.bestNexthop);
  }
  const thrift::PrefixEntry* bestEntry = nullptr;
  for (const auto& a : annsAt(p)) {
    if (a.id == r.bestOf(p)) {
      bestEntry = &a.entry;
    }
  }
  if (!bestEntry) {
    throw std::logic_error("AllNodesRouteTable: best announcer not in the prefix");
  }
  return RibUnicastEntry(prefixAt(p), std::move(nhs), *bestEntry, area_);
}

std::unordered_map<thrift::IpPrefix, RibUnicastEntry> AllNodesRouteTable::routes(
    const std::string& node) const {
  std::unordered_map<thrift::IpPrefix, RibUnicastEntry> out;
  auto it = ids_.find(node);
  if (it == ids_.end() || (prefixes_.empty() && !spare_)) {
    return out;
  }
  const Row r = fetchRow(it->second);
  for (size_t p = 0; p < numCols(); ++p) {
    if (isUni(p) && r.metricOf(p) != 0xFFFFFFFFu) {
      out.emplace(prefixAt(p), materialise(node, it->second, r, p));
    }
  }
  return out;
}

std::optional<RibMplsEntry> AllNodesRouteTable::nodeLabelEntry(
    uint32_t i, const Row& r, int32_t label) const {
  auto lc = labelCols_.find(label);
  if (lc == labelCols_.end()) {
    return std::nullopt;
  }
  // the smallest-named owner that is this node (POP_AND_LOOKUP) or that it
  // reaches (an unreachable owner inserts nothing and blocks nothing)
  for (const uint32_t col : lc->second) {
    const LabelOwner& o = owners_[col - prefixes_.size()];
    if (o.id == i) {
      thrift::NextHopThrift nh;
      nh.address.addr = std::string(16, '\0'); // "::"
      nh.area = area_;
      nh.mplsAction = createMplsAction(thrift::MplsActionCode::POP_AND_LOOKUP);
      return RibMplsEntry(label, {nh});
    }
    if (r.metricOf(col) == 0xFFFFFFFFu) {
      continue;
    }
    const std::string& node = names_[i];
    const std::string& owner = names_[o.id];
    return RibMplsEntry(label, cellNextHops(i, r, col, [&](const Link& l, int32_t metric) {
      const bool php = l.getOtherNodeName(node) == owner;
      return createNextHop(
          l.getNhV6FromNode(node), l.getIfaceFromNode(node), metric,
          createMplsAction(
              php ? thrift::MplsActionCode::PHP : thrift::MplsActionCode::SWAP,
              php ? std::nullopt : std::optional<int32_t>(label)),
          false, l.getArea());
    }));
  }
  return std::nullopt;
}

std::optional<RibMplsEntry> AllNodesRouteTable::mplsEntry(
    uint32_t i, const Row& r, int32_t label) const {
  return mplsEntryWith(i, r, label, adjLabels_[i]);
}

std::optional<RibMplsEntry> AllNodesRouteTable::mplsEntryWith(
    uint32_t i, const Row& r, int32_t label, const std::vector<AdjLabel>& adj) const {
  if (auto e = nodeLabelEntry(i, r, label)) {
    return e;
  }
  for (const AdjLabel& a : adj) {
    if (a.label == label) {
      return RibMplsEntry(
          label,
          {createNextHop(a.nhV6, a.iface, a.metric, createMplsAction(thrift::MplsActionCode::PHP),
                         false, a.area)});
    }
  }
  return std::nullopt;
}

std::unordered_map<int32_t, RibMplsEntry> AllNodesRouteTable::mplsRoutes(
    const std::string& node) const {
  std::unordered_map<int32_t, RibMplsEntry> out;
  auto it = ids_.find(node);
  if (it == ids_.end()) {
    return out;
  }
  const uint32_t i = it->second;
  const Row r = owners_.empty() ? Row{} : fetchRow(i);
  for (const auto& [label, cols] : labelCols_) {
    if (auto e = nodeLabelEntry(i, r, label)) {
      out.emplace(label, std::move(*e));
    }
  }
  for (const AdjLabel& a : adjLabels_[i]) {
    if (!out.count(a.label)) {
      out.emplace(a.label, *mplsEntry(i, r, a.label));
    }
  }
  return out;
}

// what a host-selected BGP column puts into every route of the column
// (bestArea is not part of RibUnicastEntry equality)
bool AllNodesRouteTable::sameSelection(const BgpSel& a, const BgpSel& b) {
  return a.bestEntry == b.bestEntry && a.bestNexthop == b.bestNexthop;
}

std::vector<uint32_t> AllNodesRouteTable::diff(const AllNodesRouteTable& older) {
  bool sameOwners = older.owners_.size() == owners_.size();
  for (size_t k = 0; sameOwners && k < owners_.size(); ++k) {
    sameOwners = older.owners_[k].label == owners_[k].label && older.owners_[k].id == owners_[k].id;
  }
  if (older.lfa_ != lfa_ || older.area_ != area_) {
    throw std::invalid_argument("AllNodesRouteTable::diff: different areas or LFA modes");
  }
  if (older.bgpColumns_ != bgpColumns_ || older.bgpDryRun_ != bgpDryRun_ ||
      older.bgpIgp_ != bgpIgp_) {
    // doNotInstall would flip every BGP route; a selected and a host-selected
    // column are not comparable cell by cell
    throw std::invalid_argument(
        "AllNodesRouteTable::diff: different bgpColumns, bgpDryRun or bgpUseIgpMetric");
  }
  // spare or freed columns: unicast columns pair by prefix, a free one with none
  // (a down half-edge has no counterpart, whatever the other table holds at
  // its position: the maps say so)
  if (older.names_ != names_ || holes_ || older.holes_ || older.prefixes_ != prefixes_ ||
      older.row_ != row_ || !sameOwners || downLinks_ || older.downLinks_) {
    return diffMapped(older);
  }
  // a changed PrefixEntry of a kept announcer changes routes whose cells are
  // equal: only the mapped diff (dirty announcers) sees it
  for (size_t p = 0; p < prefixes_.size(); ++p) {
    for (const auto& a : announcers_[p]) {
      for (const auto& o : older.announcers_[p]) {
        if (o.id == a.id && !(o.entry == a.entry)) {
          return diffMapped(older);
        }
      }
    }
    // BGP columns: another kind of column, another host-side selection or
    // other candidates (their order, pair codes or loopbacks) likewise
    if (columnKind(p) != older.columnKind(p)) {
      return diffMapped(older);
    }
    if (bgp_[p] || sel_[p]) {
      bool same = announcers_[p].size() == older.announcers_[p].size();
      for (size_t c = 0; same && c < announcers_[p].size(); ++c) {
        same = announcers_[p][c].id == older.announcers_[p][c].id;
      }
      if (same && bgp_[p]) {
        same = sameSelection(*bgp_[p], *older.bgp_[p]);
      }
      if (same && sel_[p]) {
        same = sel_[p]->pair == older.sel_[p]->pair && sel_[p]->via == older.sel_[p]->via;
      }
      if (!same) {
        return diffMapped(older);
      }
    }
  }
  std::vector<uint32_t> changed(names_.size());
  const auto tp = std::chrono::steady_clock::now();
  if (int s = spf_route_table_diff(older.table_.get(), table_.get(), changed.data()); s != SPF_OK) {
    if (s == SPF_E_UNSUPPORTED) {
      // same row offsets, other neighbours behind them (a link moved)
      return diffMapped(older);
    }
    tableFailure("spf_route_table_diff", s);
  }
  diffCallMs_ = (float)usSince(tp) / 1000.f;
  diffed_ = true;
  mapped_ = false;
  goneCols_.clear();
  goneNew_.clear();
  rowOf_.resize(names_.size());
  for (uint32_t i = 0; i < rowOf_.size(); ++i) {
    rowOf_[i] = i;
  }
  older_ = &older;
  patchDelta_ = false;
  topoDelta_ = false;
  return changed;
}

std::vector<uint32_t> AllNodesRouteTable::diffMapped(const AllNodesRouteTable& older) {
  const uint32_t V = (uint32_t)names_.size(), Va = (uint32_t)older.names_.size();
  const size_t P = prefixes_.size(), C = numCols();
  const size_t Pa = older.prefixes_.size(), Ca = older.numCols();
  // rows and best announcers: by node name
  std::vector<uint32_t> rowOf(V, SPF_MAP_NONE), nodeOf(Va, SPF_MAP_NONE);
  for (uint32_t i = 0; i < V; ++i) {
    auto it = older.ids_.find(names_[i]);
    if (it != older.ids_.end()) {
      rowOf[i] = it->second;
      nodeOf[it->second] = i;
    }
  }
  // columns: unicast by prefix, node labels by (label, owner name)
  std::vector<uint32_t> colOf(C, SPF_MAP_NONE), gone, goneNew;
  std::unordered_map<uint32_t, uint32_t> newOfOld; // older column -> newer one of another kind
  std::vector<uint8_t> kept(Ca, 0);
  {
    std::unordered_map<thrift::IpPrefix, uint32_t> colA;
    colA.reserve(Pa);
    // (a free column serves no prefix: no counterpart, and no route on either side)
    for (uint32_t p = 0; p < Ca; ++p) {
      if (older.isUni(p) && !older.isFree(p)) {
        colA.emplace(older.prefixAt(p), p);
      }
    }
    for (size_t p = 0; p < C; ++p) {
      if (!isUni(p) || isFree(p)) {
        continue;
      }
      auto it = colA.find(prefixAt(p));
      if (it == colA.end()) {
        continue;
      }
      if (columnKind(p) != older.columnKind(it->second)) {
        // Open/R, host-selected BGP, selected: another kind of column has no
        // counterpart -- the older one is gone, and a node with a route on
        // both sides gets one update (unicastDelta drops the delete)
        newOfOld.emplace(it->second, (uint32_t)p);
        continue;
      }
      colOf[p] = it->second;
      kept[it->second] = 1;
    }
    std::map<std::pair<int32_t, uint32_t>, uint32_t> labA; // (label, newer owner id) -> column
    for (size_t k = 0; k < older.owners_.size(); ++k) {
      const uint32_t id = nodeOf[older.owners_[k].id];
      if (id != SPF_MAP_NONE) {
        labA.emplace(std::make_pair(older.owners_[k].label, id), (uint32_t)(Pa + k));
      }
    }
    for (size_t k = 0; k < owners_.size(); ++k) {
      auto it = labA.find({owners_[k].label, owners_[k].id});
      if (it != labA.end()) {
        colOf[P + k] = it->second;
        kept[it->second] = 1;
      }
    }
    for (uint32_t c = 0; c < Ca; ++c) {
      if (!kept[c]) {
        gone.push_back(c);
        auto it = newOfOld.find(c);
        goneNew.push_back(it == newOfOld.end() ? SPF_MAP_NONE : it->second);
      }
    }
  }
  // links: by Link identity (node and interface names); a link whose
  // next-hop addresses, interface or area differ from this node has no
  // counterpart.  Rows whose links all keep their positions get an empty
  // segment (identity).
  std::vector<uint32_t> linkOff(V + 1, 0), linkOf;
  {
    auto same = [](const Link& a, const Link& b, const std::string& node) {
      return a == b && a.getArea() == b.getArea() &&
          a.getIfaceFromNode(node) == b.getIfaceFromNode(node) &&
          a.getNhV4FromNode(node) == b.getNhV4FromNode(node) &&
          a.getNhV6FromNode(node) == b.getNhV6FromNode(node);
    };
    std::unordered_multimap<size_t, uint32_t> byHash;
    for (uint32_t i = 0; i < V; ++i) {
      linkOff[i + 1] = linkOff[i];
      const uint32_t ia = rowOf[i];
      if (ia == SPF_MAP_NONE) {
        continue;
      }
      const uint32_t e0 = row_[i], deg = row_[i + 1] - e0;
      const uint32_t a0 = older.row_[ia], dega = older.row_[ia + 1] - a0;
      // (a half-edge that is down, applyTopologyChanges with linksInPlace, is
      // no link of its table: no counterpart on either side)
      bool ident = deg == dega;
      for (uint32_t j = 0; ident && j < deg; ++j) {
        ident = !isDown(e0 + j) && !older.isDown(a0 + j) &&
            same(*halfLink_[e0 + j], *older.halfLink_[a0 + j], names_[i]);
      }
      if (ident) {
        continue;
      }
      byHash.clear();
      for (uint32_t j = 0; j < dega; ++j) {
        if (!older.isDown(a0 + j)) {
          byHash.emplace(older.halfLink_[a0 + j]->hash, j);
        }
      }
      for (uint32_t j = 0; j < deg; ++j) {
        uint32_t t = SPF_MAP_NONE;
        const Link& l = *halfLink_[e0 + j];
        auto [lo, hi] = byHash.equal_range(l.hash);
        if (isDown(e0 + j)) {
          hi = lo;
        }
        for (auto it = lo; it != hi; ++it) {
          if (same(l, *older.halfLink_[a0 + it->second], names_[i])) {
            t = it->second;
            byHash.erase(it); // (a link is one bit of the row: injective)
            break;
          }
        }
        linkOf.push_back(t);
      }
      linkOff[i + 1] = (uint32_t)linkOf.size();
    }
  }
  // dirty announcers: same node, PrefixEntry unequal.  A BGP column selected
  // on the host has the selection's best entry and loopback at every node:
  // if either differs every announcer is dirty (the cell's best is one of
  // them, so every routed cell is an update); the cell's own best is no part
  // of its routes (the SPF_MAP_NONE entry).  A candidate of a selected column
  // is dirty when its entry or its loopback differs.
  std::vector<uint32_t> dirtyOff(C + 1, 0), dirtyAnn;
  for (size_t p = 0; p < C; ++p) {
    if (isUni(p) && colOf[p] != SPF_MAP_NONE) {
      const uint32_t pa = colOf[p];
      const auto& olds = older.annsAt(pa);
      const auto& news = annsAt(p);
      if (columnKind(p) == 1) {
        dirtyAnn.push_back(SPF_MAP_NONE);
        if (!sameSelection(bgpAt(p), older.bgpAt(pa))) {
          for (const auto& a : news) {
            dirtyAnn.push_back(a.id);
          }
        }
      } else if (columnKind(p) == 0 && !olds.empty() && !news.empty() &&
                 !(olds.size() == 1 && news.size() == 1 && nodeOf[olds[0].id] == news[0].id) &&
                 std::all_of(olds.begin(), olds.end(), [&](const Announcer& o) {
                   return o.entry == olds[0].entry;
                 })) {
        // several announcers (or another one) with ONE PrefixEntry on the
        // older side: bestPrefixEntry was that entry whoever was best, so a
        // route's entry changed iff the newer best's differs from it -- not
        // when `best` moves between equal entries (an anycast gaining an
        // announcer).  The cell's best is not compared (SPF_MAP_NONE).
        dirtyAnn.push_back(SPF_MAP_NONE);
        for (const auto& a : news) {
          if (!(a.entry == olds[0].entry)) {
            dirtyAnn.push_back(a.id);
          }
        }
      } else {
        for (size_t c = 0; c < news.size(); ++c) {
          const auto& a = news[c];
          for (size_t b = 0; b < olds.size(); ++b) {
            const auto& o = olds[b];
            if (nodeOf[o.id] == a.id &&
                (!(o.entry == a.entry) ||
                 (columnKind(p) == 2 && !(selAt(p).via[c] == older.selAt(pa).via[b])))) {
              dirtyAnn.push_back(a.id);
            }
          }
        }
      }
    }
    dirtyOff[p + 1] = (uint32_t)dirtyAnn.size();
  }
  // identity maps go as null arrays: the kernel then skips their loads (on a
  // link flap every map but two rows' link_of is the identity)
  bool sameRows = V == Va, sameCols = C == Ca;
  for (uint32_t i = 0; sameRows && i < V; ++i) {
    sameRows = rowOf[i] == i;
  }
  for (size_t p = 0; sameCols && p < C; ++p) {
    sameCols = colOf[p] == p;
  }
  spf_route_diff_map m{};
  m.row_of = sameRows ? nullptr : rowOf.data();
  m.col_of = sameCols ? nullptr : colOf.data();
  m.gone_cols = gone.data();
  m.num_gone = (uint32_t)gone.size();
  m.node_of = sameRows ? nullptr : nodeOf.data();
  m.link_off = linkOf.empty() ? nullptr : linkOff.data();
  m.link_of = linkOf.data();
  m.dirty_off = dirtyAnn.empty() ? nullptr : dirtyOff.data();
  m.dirty_ann = dirtyAnn.data();
  std::vector<uint32_t> changed(V);
  const auto tp = std::chrono::steady_clock::now();
  if (int s = spf_route_table_diff_mapped(older.table_.get(), table_.get(), &m, changed.data());
      s != SPF_OK) {
    if (s == SPF_E_UNSUPPORTED) {
      throw std::invalid_argument(std::string("AllNodesRouteTable::diff: ") +
                                  spf_last_error_detail());
    }
    tableFailure("spf_route_table_diff_mapped", s);
  }
  diffCallMs_ = (float)usSince(tp) / 1000.f;
  // a column that changed its kind: a node with a route on both sides was
  // counted twice (gone + new) and gets one update
  std::vector<uint32_t> rows, colsNew, colsOld;
  for (size_t g = 0; g < gone.size(); ++g) {
    for (uint32_t i = 0; goneNew[g] != SPF_MAP_NONE && i < V; ++i) {
      if (rowOf[i] != SPF_MAP_NONE) {
        rows.push_back(i);
        colsNew.push_back(goneNew[g]);
        colsOld.push_back(gone[g]);
      }
    }
  }
  if (!rows.empty()) {
    auto routed = [](const AllNodesRouteTable& t, const std::vector<uint32_t>& rs,
                         const std::vector<uint32_t>& cs) {
      uint64_t nl = 0, nm = 0;
      for (const uint32_t r : rs) {
        const uint64_t deg = t.row_[r + 1] - t.row_[r];
        nl += (deg + 63) / 64;
        nm += t.lfa_ ? deg : 0;
      }
      std::vector<uint32_t> metric(rs.size()), best(rs.size()), lmet(std::max<uint64_t>(nm, 1));
      std::vector<uint64_t> links(std::max<uint64_t>(nl, 1));
      if (int s = spf_route_table_fetch_cells(
              t.table_.get(), rs.size(), rs.data(), cs.data(), metric.data(), best.data(),
              links.data(), t.lfa_ ? lmet.data() : nullptr);
          s != SPF_OK) {
        tableFailure("spf_route_table_fetch_cells", s);
      }
      return metric;
    };
    std::vector<uint32_t> oldRows(rows.size());
    for (size_t k = 0; k < rows.size(); ++k) {
      oldRows[k] = rowOf[rows[k]];
    }
    const auto mn = routed(*this, rows, colsNew);
    const auto mo = routed(older, oldRows, colsOld);
    for (size_t k = 0; k < rows.size(); ++k) {
      if (mn[k] != 0xFFFFFFFFu && mo[k] != 0xFFFFFFFFu) {
        changed[rows[k]] -= 1;
      }
    }
  }
  diffed_ = true;
  mapped_ = true;
  rowOf_ = std::move(rowOf);
  goneCols_ = std::move(gone);
  goneNew_ = std::move(goneNew);
  older_ = &older;
  patchDelta_ = false;
  topoDelta_ = false;
  return changed;
}

// prefixes() once the columns have holes: the served unicast columns in
// column order, and their index by prefix
void AllNodesRouteTable::rebuildServed() {
  holes_ = true;
  if (free_.empty()) {
    free_.assign(prefixes_.size() + spare_ + spareSel_, 0);
  }
  served_.clear();
  colOfPrefix_.clear();
  for (size_t c = 0; c < numCols(); ++c) {
    if (isUni(c) && !isFree(c)) {
      served_.push_back(prefixAt(c));
      colOfPrefix_.emplace(prefixAt(c), (uint32_t)c);
    }
  }
}

std::vector<uint32_t> AllNodesRouteTable::applyPrefixChanges(
    const PrefixState& ps, const std::unordered_set<thrift::IpPrefix>& changed) {
  if ((bgpColumns_ && !bgpInPlace_) || hasBorder_) {
    throw std::invalid_argument(
        "AllNodesRouteTable::applyPrefixChanges: tables with bgpColumns or borderNodes are "
        "rebuilt (BGP columns and per-area served sets do not move in place)");
  }
  const auto tp = std::chrono::steady_clock::now();
  if (!holes_) {
    rebuildServed(); // (the index by prefix; no column is free yet)
  }
  // rescan every changed prefix with the constructor's rules
  static const thrift::PrefixEntries kNoEntries;
  PrefixScan scan{nullptr, ps, nullptr, bgpColumns_, bgpIgp_};
  for (const auto& prefix : changed) {
    auto it = ps.prefixes().find(prefix);
    scan.items.emplace_back(&prefix, it == ps.prefixes().end() ? &kNoEntries : &it->second);
  }
  if (bgpColumns_) {
    // A BGP route holds the loopback of its best announcer
    // (PrefixState::getLoopbackVias), which is another prefix of that node:
    // every served BGP prefix with an announcer that announces, or announced,
    // a changed prefix is rescanned too (an unchanged one patches to no bits)
    std::unordered_set<std::string> touched;
    for (const auto& [prefix, entries] : scan.items) {
      for (const auto& [node, byArea] : *entries) {
        touched.insert(node);
      }
      if (auto it = colOfPrefix_.find(*prefix); it != colOfPrefix_.end()) {
        for (const auto& a : annsAt(it->second)) {
          touched.insert(names_[a.id]);
        }
      }
    }
    for (size_t c = 0; c < numCols(); ++c) {
      if (!isUni(c) || isFree(c) || columnKind(c) == 0 || changed.count(prefixAt(c))) {
        continue;
      }
      auto it = ps.prefixes().find(prefixAt(c));
      if (it != ps.prefixes().end() &&
          std::any_of(it->second.begin(), it->second.end(),
                      [&](const auto& kv) { return touched.count(kv.first) > 0; })) {
        scan.items.emplace_back(&it->first, &it->second);
      }
    }
  }
  const size_t n = scan.items.size();
  scan.keep.assign(n, 0);
  scan.anns.resize(n);
  scan.sels.resize(n);
  scan.selCols.resize(n);
  scan.bgpAll.resize(n);
  for (size_t i = 0; i < n; ++i) {
    scanPrefix(scan, i);
  }
  if (bgpColumns_ && !bgpIgp_) {
    dropUnreachableBgp(scan); // (on the resident rows)
  }
  // classify; nothing is touched before every new prefix has a column.  A
  // prefix keeps its column unless it needs the other kind of device column
  // (selected / unselected): then the old one is emptied and it moves
  std::vector<uint32_t> colFor(n, SPF_MAP_NONE);
  std::vector<uint8_t> moves(n, 0);
  size_t need = 0, needSel = 0;
  for (size_t i = 0; i < n; ++i) {
    const bool wantSel = scan.keep[i] == 3;
    auto it = colOfPrefix_.find(*scan.items[i].first);
    if (it != colOfPrefix_.end()) {
      colFor[i] = it->second;
      moves[i] = scan.keep[i] != 0 && selectedColumn(it->second) != wantSel;
    }
    if (scan.keep[i] && (colFor[i] == SPF_MAP_NONE || moves[i])) {
      (wantSel ? needSel : need) += 1;
    }
  }
  if (need > freeList_.size() || needSel > freeSelList_.size()) {
    throw std::length_error(
        "AllNodesRouteTable::applyPrefixChanges: " + std::to_string(need) + " + " +
        std::to_string(needSel) + " new prefixes, " + std::to_string(freeList_.size()) + " + " +
        std::to_string(freeSelList_.size()) +
        " free columns (unselected + selected; rebuild the table)");
  }
  // the listed columns: column, its changed prefix, and whether it serves the
  // prefix after the call (else it is emptied)
  struct Listed {
    uint32_t col;
    size_t item;
    bool serve;
  };
  std::vector<Listed> listed;
  std::vector<std::pair<uint32_t, uint32_t>> moved; // (emptied column, column taken) of one prefix
  std::vector<uint32_t> taken;                      // popped from the free lists
  for (size_t i = 0; i < n; ++i) {
    const bool had = colFor[i] != SPF_MAP_NONE;
    if (!had && !scan.keep[i]) {
      continue; // not served before or now
    }
    if (had && (!scan.keep[i] || moves[i])) {
      listed.push_back(Listed{colFor[i], i, false});
    }
    if (scan.keep[i] && (!had || moves[i])) {
      // (freed columns lie behind the spare ones: reused first)
      auto& fl = scan.keep[i] == 3 ? freeSelList_ : freeList_;
      const uint32_t c = fl.back();
      fl.pop_back();
      taken.push_back(c);
      if (had) {
        moved.emplace_back(colFor[i], c);
      }
      listed.push_back(Listed{c, i, true});
    } else if (scan.keep[i]) {
      listed.push_back(Listed{colFor[i], i, true});
    }
  }
  std::vector<uint32_t> cols, annOff{0}, ann, dirtyOff{0}, dirtyAnn;
  std::vector<uint8_t> candFlags;
  std::vector<uint32_t> selColumns;
  std::vector<uint64_t> pairOff{0};
  std::vector<uint16_t> pairCodes;
  for (const Listed& l : listed) {
    const size_t i = l.item;
    const int newKind = (int)scan.keep[i] - 1;
    static const std::vector<Announcer> kNone;
    const auto& news = l.serve ? scan.anns[i] : kNone;
    if (l.serve && !isFree(l.col)) {
      const auto& olds = annsAt(l.col);
      const int oldKind = columnKind(l.col);
      if (oldKind != newKind) {
        // Open/R <-> host-selected BGP in one column: every route is another one
        for (const auto& a : news) {
          dirtyAnn.push_back(a.id);
        }
      } else if (newKind == 1) {
        if (!sameSelection(bgpAt(l.col), *scan.sels[i])) {
          for (const auto& a : news) {
            dirtyAnn.push_back(a.id);
          }
        }
      } else {
        // kept announcers whose PrefixEntry (selected columns: or loopback)
        // differs (the rule of diffMapped)
        for (size_t c = 0; c < news.size(); ++c) {
          for (size_t o = 0; o < olds.size(); ++o) {
            if (olds[o].id == news[c].id &&
                (!(olds[o].entry == news[c].entry) ||
                 (newKind == 2 && !(selAt(l.col).via[o] == scan.selCols[i]->via[c])))) {
              dirtyAnn.push_back(news[c].id);
            }
          }
        }
      }
      if (newKind == 1) {
        dirtyAnn.push_back(SPF_MAP_NONE); // the cell's own best is no part of its routes
      }
    }
    if (selectedColumn(l.col)) {
      selColumns.push_back(l.col);
      if (l.serve) {
        const SelCol& sc = *scan.selCols[i];
        pairCodes.insert(pairCodes.end(), sc.pair.begin(), sc.pair.end());
      }
      pairOff.push_back(pairCodes.size());
    }
    cols.push_back(l.col);
    for (size_t c = 0; c < news.size(); ++c) {
      ann.push_back(news[c].id);
      candFlags.push_back(newKind == 2 && scan.selCols[i]->via[c] ? 1 : 0);
    }
    annOff.push_back((uint32_t)ann.size());
    dirtyOff.push_back((uint32_t)dirtyAnn.size());
  }
  // A kept Open/R column whose announcer set changed: `best` can move between
  // two announcers with EQUAL PrefixEntries, which the device reports (best is
  // a cell word) and getRouteDelta does not (bestPrefixEntry is the same).  The
  // cells of those columns are read before and after the patch and such
  // cells taken out of this call's delta (suppress_).  A kept selected column
  // likewise: its best can move with the same candidates (other pair codes),
  // and the route is the same only where the old and the new best candidate
  // have equal entries AND equal loopbacks and the cell's igp word stayed.
  // (Host-selected BGP columns do not compare best.)
  const uint32_t V = (uint32_t)names_.size();
  std::vector<size_t> risk; // indices into listed
  std::vector<std::vector<Announcer>> riskOld;
  std::vector<std::vector<std::optional<thrift::NextHopThrift>>> riskOldVia; // (selected columns)
  bool riskSel = false;
  for (size_t k = 0; k < listed.size(); ++k) {
    const Listed& l = listed[k];
    if (!l.serve || isFree(l.col)) {
      continue;
    }
    const bool plain = columnKind(l.col) == 0 && scan.keep[l.item] == 1;
    const bool selected = columnKind(l.col) == 2 && scan.keep[l.item] == 3;
    if (!plain && !selected) {
      continue;
    }
    const auto& olds = annsAt(l.col);
    const auto& news = scan.anns[l.item];
    if (news.empty() || olds.empty()) {
      continue;
    }
    bool sameIds = olds.size() == news.size();
    for (size_t c = 0; sameIds && c < news.size(); ++c) {
      sameIds = olds[c].id == news[c].id;
    }
    // (a selected column: only where some old and some other new candidate
    // have equal entries and equal loopbacks can a moved best leave the route
    // equal -- else no cell can be left out and the reads are saved)
    bool twins = false;
    for (size_t o = 0; selected && !twins && o < olds.size(); ++o) {
      for (size_t c = 0; !twins && c < news.size(); ++c) {
        twins = olds[o].id != news[c].id && olds[o].entry == news[c].entry &&
            selAt(l.col).via[o] == scan.selCols[l.item]->via[c];
      }
    }
    if (selected ? twins : !sameIds) {
      risk.push_back(k);
      riskOld.push_back(olds);
      riskOldVia.push_back(selected ? selAt(l.col).via
                                    : std::vector<std::optional<thrift::NextHopThrift>>{});
      riskSel |= selected;
    }
  }
  struct CellList {
    std::vector<uint32_t> metric, best, lmet, igp;
    std::vector<uint64_t> links;
  };
  // the cells (every row) x (the given columns), row-major
  auto readCells = [&](const std::vector<uint32_t>& cs) {
    CellList c;
    std::vector<uint32_t> rows, ccols;
    uint64_t lw = 0, lm = 0;
    for (uint32_t i = 0; i < V; ++i) {
      const uint64_t deg = row_[i + 1] - row_[i];
      for (const uint32_t x : cs) {
        rows.push_back(i);
        ccols.push_back(x);
        lw += (deg + 63) / 64;
        lm += lfa_ ? deg : 0;
      }
    }
    c.metric.resize(rows.size());
    c.best.resize(rows.size());
    c.links.resize(std::max<uint64_t>(lw, 1));
    c.lmet.resize(std::max<uint64_t>(lm, 1));
    if (int s = spf_route_table_fetch_cells(
            table_.get(), rows.size(), rows.data(), ccols.data(), c.metric.data(), c.best.data(),
            c.links.data(), lfa_ ? c.lmet.data() : nullptr);
        s != SPF_OK) {
      tableFailure("spf_route_table_fetch_cells", s);
    }
    if (riskSel) {
      c.igp.resize(rows.size());
      if (int s = spf_route_table_fetch_cells_igp(table_.get(), rows.size(), rows.data(),
                                                  ccols.data(), c.igp.data());
          s != SPF_OK) {
        tableFailure("spf_route_table_fetch_cells_igp", s);
      }
    }
    return c;
  };
  std::vector<uint32_t> riskCols, movedFrom, movedTo;
  for (const size_t k : risk) {
    riskCols.push_back(listed[k].col);
  }
  for (const auto& [from, to] : moved) {
    movedFrom.push_back(from);
    movedTo.push_back(to);
  }
  const CellList riskBefore = risk.empty() ? CellList{} : readCells(riskCols);
  const CellList movedBefore = moved.empty() ? CellList{} : readCells(movedFrom);
  spf_route_patch patch{};
  patch.num_columns = (uint32_t)cols.size();
  patch.columns = cols.data();
  patch.ann_offsets = annOff.data();
  patch.announcers = ann.data();
  patch.dirty_off = dirtyAnn.empty() ? nullptr : dirtyOff.data();
  patch.dirty_ann = dirtyAnn.data();
  spf_route_select_desc sd{};
  sd.num_selected = (uint32_t)selColumns.size();
  sd.columns = selColumns.data();
  sd.pair_offsets = pairOff.data();
  sd.pair_codes = pairCodes.data();
  candFlags.push_back(0); // (never a null array)
  sd.cand_flags = candFlags.data();
  std::vector<uint32_t> counts(names_.size());
  const int st = bgpColumns_
      ? spf_route_table_patch_columns_sel(table_.get(), &patch, selColumns.empty() ? nullptr : &sd,
                                          counts.data())
      : spf_route_table_patch_columns(table_.get(), &patch, counts.data());
  if (st != SPF_OK) {
    // (the engine checked before it touched anything: give the columns back)
    for (size_t k = taken.size(); k-- > 0;) {
      (selectedColumn(taken[k]) ? freeSelList_ : freeList_).push_back(taken[k]);
    }
    tableFailure("spf_route_table_patch_columns", st);
  }
  if (int s = spf_route_table_patch_elapsed_ms(table_.get(), &patchMs_); s != SPF_OK) {
    tableFailure("spf_route_table_patch_elapsed_ms", s);
  }
  suppress_.assign(V, {});
  if (!risk.empty()) {
    const CellList after = readCells(riskCols);
    auto entryOf = [](const std::vector<Announcer>& as, uint32_t id) -> const thrift::PrefixEntry* {
      for (const auto& a : as) {
        if (a.id == id) {
          return &a.entry;
        }
      }
      return nullptr;
    };
    size_t x = 0;
    uint64_t lw = 0, lm = 0;
    for (uint32_t i = 0; i < V; ++i) {
      const uint64_t deg = row_[i + 1] - row_[i], W = (deg + 63) / 64, M = lfa_ ? deg : 0;
      for (size_t r = 0; r < risk.size(); ++r, ++x, lw += W, lm += M) {
        const uint32_t ob = riskBefore.best[x], nb = after.best[x];
        if (riskBefore.metric[x] == 0xFFFFFFFFu || after.metric[x] == 0xFFFFFFFFu || ob == nb) {
          continue;
        }
        const auto& news = scan.anns[listed[risk[r]].item];
        const auto* oe = entryOf(riskOld[r], ob);
        const auto* ne = entryOf(news, nb);
        if (!oe || !ne || !(*oe == *ne)) {
          continue;
        }
        if (!riskOldVia[r].empty()) {
          // a selected column: the best candidate's loopback and the igp word
          // are the route's bestNexthop
          const auto& nvia = scan.selCols[listed[risk[r]].item]->via;
          size_t oi = 0, ni = 0; // (oe and ne were found: both ids are in their lists)
          while (riskOld[r][oi].id != ob) {
            ++oi;
          }
          while (news[ni].id != nb) {
            ++ni;
          }
          if (!(riskOldVia[r][oi] == nvia[ni]) || riskBefore.igp[x] != after.igp[x]) {
            continue;
          }
        } else {
          const auto* neOld = entryOf(riskOld[r], nb); // (the new best, if it was an announcer: dirty?)
          if (neOld && !(*neOld == *ne)) {
            continue;
          }
        }
        if ((!lfa_ && riskBefore.metric[x] != after.metric[x]) ||
            !std::equal(after.links.begin() + lw, after.links.begin() + lw + W,
                        riskBefore.links.begin() + lw) ||
            !std::equal(after.lmet.begin() + lm, after.lmet.begin() + lm + M,
                        riskBefore.lmet.begin() + lm)) {
          continue;
        }
        suppress_[i].push_back(riskCols[r]); // only `best` moved, onto an equal entry
      }
    }
  }
  if (!moved.empty()) {
    // a prefix that moved to the other kind of column: a node with a route
    // before and after gets ONE update (getRouteDelta), so the emptied
    // column's delete is taken out there
    const CellList after = readCells(movedTo);
    size_t x = 0;
    for (uint32_t i = 0; i < V; ++i) {
      for (size_t r = 0; r < moved.size(); ++r, ++x) {
        if (movedBefore.metric[x] != 0xFFFFFFFFu && after.metric[x] != 0xFFFFFFFFu) {
          suppress_[i].push_back(movedFrom[r]);
        }
      }
    }
  }
  for (uint32_t i = 0; i < V; ++i) {
    std::sort(suppress_[i].begin(), suppress_[i].end());
    counts[i] -= (uint32_t)suppress_[i].size();
  }
  // the host's view of the columns (emptied ones first: a moved prefix's new
  // column is listed after its old one)
  for (const Listed& l : listed) {
    const uint32_t c = l.col;
    const size_t i = l.item, slot = slotOf(c);
    if (!l.serve) {
      (selectedColumn(c) ? freeSelList_ : freeList_).push_back(c);
    }
    free_[slot] = l.serve ? 0 : 1;
    // (a freed column keeps its prefix: this call's delta names it in the delete)
    auto& as = c < prefixes_.size() ? announcers_[c] : spareAnn_[c - spareBase()];
    if (l.serve) {
      (c < prefixes_.size() ? prefixes_[c] : sparePrefix_[c - spareBase()]) = *scan.items[i].first;
      as = std::move(scan.anns[i]);
    } else {
      as.clear();
    }
    if (slot < bgp_.size()) {
      bgp_[slot] = l.serve && scan.keep[i] == 2 ? std::move(scan.sels[i]) : std::nullopt;
      sel_[slot] = l.serve && scan.keep[i] == 3 ? std::move(scan.selCols[i]) : std::nullopt;
    }
  }
  rebuildServed();
  if (bgpColumns_) {
    nbgp_ = nsel_ = 0;
    for (size_t c = 0; c < numCols(); ++c) {
      if (isUni(c) && !isFree(c)) {
        nbgp_ += columnKind(c) >= 1;
        nsel_ += columnKind(c) == 2;
      }
    }
  }
  diffed_ = true;
  mapped_ = false;
  patchDelta_ = true;
  topoDelta_ = false;
  older_ = nullptr;
  goneCols_.clear();
  goneNew_.clear();
  rowOf_.resize(names_.size());
  for (uint32_t i = 0; i < rowOf_.size(); ++i) {
    rowOf_[i] = i;
  }
  Counters::add("decision.route_table_patch_us", usSince(tp));
  return counts;
}

std::vector<uint32_t> routeRefreshRowList(
    const std::vector<uint8_t>& affected, const std::vector<uint32_t>& row,
    const std::vector<uint32_t>& col, const std::vector<uint32_t>& changedTails, bool lfa) {
  const size_t V = affected.size();
  if (row.size() != V + 1 || (V && row[V] > col.size())) {
    throw std::invalid_argument("routeRefreshRowList: the CSR does not match the nodes");
  }
  std::vector<uint8_t> listed(affected.begin(), affected.end());
  if (lfa) {
    for (size_t i = 0; i < V; ++i) {
      for (uint32_t e = row[i]; e < row[i + 1] && !listed[i]; ++e) {
        listed[i] = col[e] < V && affected[col[e]];
      }
    }
    for (const uint32_t t : changedTails) {
      listed.at(t) = 1;
    }
  }
  std::vector<uint32_t> out;
  for (size_t i = 0; i < V; ++i) {
    if (listed[i]) {
      out.push_back((uint32_t)i);
    }
  }
  return out;
}

AllNodesRouteTable::Row AllNodesRouteTable::fetchPrevRow(uint32_t i) const {
  Row r;
  const size_t P = numCols();
  r.deg = row_[i + 1] - row_[i];
  r.W = (r.deg + 63) / 64;
  r.metric.resize(P);
  r.best.resize(P);
  r.links.resize(std::max<size_t>(1, P * r.W));
  if (lfa_) {
    r.lmet.resize(std::max<size_t>(1, P * r.deg));
  }
  std::vector<uint32_t> rows(P, i), cols(P);
  for (size_t p = 0; p < P; ++p) {
    cols[p] = (uint32_t)p;
  }
  if (int s = spf_route_table_fetch_cells_prev(
          table_.get(), P, rows.data(), cols.data(), r.metric.data(), r.best.data(),
          r.links.data(), lfa_ ? r.lmet.data() : nullptr);
      s != SPF_OK) {
    tableFailure("spf_route_table_fetch_cells_prev", s);
  }
  return r;
}

void AllNodesRouteTable::refuseTopologyChanges(const char* who) const {
  if (hasBorder_) {
    throw std::invalid_argument(std::string(who) + "a table built with borderNodes");
  }
  if (bgpColumns_ && !bgpInPlace_) {
    throw std::invalid_argument(std::string(who) + "a table built with bgpColumns and without "
                                                   "bgpInPlace");
  }
  if (bgpColumns_ && !bgpIgp_) {
    // (the winners of a host-selected column depend on the drain filter and on
    // every node reaching every announcer, and reachesAll_ would go stale)
    throw std::invalid_argument(std::string(who) + "a table built with bgpColumns and without "
                                                   "bgpUseIgpMetric (host-selected BGP columns)");
  }
}

void AllNodesRouteTable::refreshListedRows(
    spf_query* q, bool all, const std::vector<uint32_t>& rows, std::vector<uint32_t>& counts) {
  // (nothing listed: an all-clear bitmap over the given query)
  const uint32_t none = 0;
  const uint32_t n = all ? 0 : (uint32_t)rows.size();
  const uint32_t* list = all ? nullptr : rows.empty() ? &none : rows.data();
  // a device table with selected columns: their fold runs again in the same pass
  if (devSel_) {
    if (int s = spf_route_table_refresh_rows_sel(table_.get(), q, n, list, counts.data());
        s != SPF_OK) {
      tableFailure("spf_route_table_refresh_rows_sel", s);
    }
    return;
  }
  if (int s = spf_route_table_refresh_rows(table_.get(), q, n, list, counts.data());
      s != SPF_OK) {
    tableFailure("spf_route_table_refresh_rows", s);
  }
}

// A metric change moves the best candidate of a selected column often (every
// candidate's vector carries its distance).  The device reports the cell
// (best is a cell word); the route is the same where the old and the new best
// candidate have equal entries AND equal loopbacks and metric (non-LFA), links,
// link metrics and the igp word all stayed -- the rule applyPrefixChanges uses
// for kept selected columns.
void AllNodesRouteTable::suppressSelectedBest(std::vector<uint32_t>& counts) {
  const uint32_t V = (uint32_t)names_.size();
  std::vector<uint32_t> risk; // selected columns that hold such a candidate pair
  for (size_t c = 0; devSel_ && c < numCols(); ++c) {
    if (!isUni(c) || isFree(c) || columnKind(c) != 2) {
      continue;
    }
    const auto& as = annsAt(c);
    const auto& via = selAt(c).via;
    bool twin = false;
    for (size_t x = 0; !twin && x < as.size(); ++x) {
      for (size_t y = x + 1; !twin && y < as.size(); ++y) {
        twin = as[x].id != as[y].id && as[x].entry == as[y].entry && via[x] == via[y];
      }
    }
    if (twin) {
      risk.push_back((uint32_t)c);
    }
  }
  if (risk.empty()) {
    return;
  }
  std::vector<uint32_t> rr, cc;
  std::vector<uint64_t> bits((numCols() + 63) / 64);
  uint64_t nl = 0, nm = 0;
  for (uint32_t i = 0; i < V; ++i) {
    if (!counts[i]) {
      continue;
    }
    if (int s = spf_route_table_changed(table_.get(), i, bits.data()); s != SPF_OK) {
      tableFailure("spf_route_table_changed", s);
    }
    const uint64_t deg = row_[i + 1] - row_[i];
    for (const uint32_t c : risk) {
      if ((bits[c / 64] >> (c % 64)) & 1) {
        rr.push_back(i);
        cc.push_back(c);
        nl += (deg + 63) / 64;
        nm += lfa_ ? deg : 0;
      }
    }
  }
  if (rr.empty()) {
    return;
  }
  struct Cells {
    std::vector<uint32_t> metric, best, lmet, igp;
    std::vector<uint64_t> links;
  };
  auto read = [&](decltype(&spf_route_table_fetch_cells) fetch,
                  decltype(&spf_route_table_fetch_cells_igp) fetchIgp, const char* what) {
    Cells z;
    z.metric.resize(rr.size());
    z.best.resize(rr.size());
    z.igp.resize(rr.size());
    z.links.resize(std::max<uint64_t>(nl, 1));
    z.lmet.resize(std::max<uint64_t>(nm, 1));
    if (int s = fetch(table_.get(), rr.size(), rr.data(), cc.data(), z.metric.data(),
                      z.best.data(), z.links.data(), lfa_ ? z.lmet.data() : nullptr);
        s != SPF_OK) {
      tableFailure(what, s);
    }
    if (int s = fetchIgp(table_.get(), rr.size(), rr.data(), cc.data(), z.igp.data());
        s != SPF_OK) {
      tableFailure(what, s);
    }
    return z;
  };
  const Cells now = read(spf_route_table_fetch_cells, spf_route_table_fetch_cells_igp,
                         "spf_route_table_fetch_cells");
  const Cells was = read(spf_route_table_fetch_cells_prev, spf_route_table_fetch_cells_prev_igp,
                         "spf_route_table_fetch_cells_prev");
  uint64_t lw = 0, lm = 0;
  std::vector<uint8_t> touched(V, 0);
  for (size_t k = 0; k < rr.size(); ++k) {
    const uint64_t deg = row_[rr[k] + 1] - row_[rr[k]], W = (deg + 63) / 64, M = lfa_ ? deg : 0;
    const uint64_t lw0 = lw, lm0 = lm;
    lw += W;
    lm += M;
    if (was.metric[k] == 0xFFFFFFFFu || now.metric[k] == 0xFFFFFFFFu ||
        was.best[k] == now.best[k] || was.igp[k] != now.igp[k]) {
      continue;
    }
    const auto& as = annsAt(cc[k]);
    const auto& via = selAt(cc[k]).via;
    size_t oi = as.size(), ni = as.size();
    for (size_t x = 0; x < as.size(); ++x) {
      oi = as[x].id == was.best[k] && oi == as.size() ? x : oi;
      ni = as[x].id == now.best[k] && ni == as.size() ? x : ni;
    }
    if (oi == as.size() || ni == as.size() || !(as[oi].entry == as[ni].entry) ||
        !(via[oi] == via[ni])) {
      continue;
    }
    // (LFA: the metric word is no part of the route, see diff())
    if ((!lfa_ && was.metric[k] != now.metric[k]) ||
        !std::equal(now.links.begin() + lw0, now.links.begin() + lw0 + W,
                    was.links.begin() + lw0) ||
        !std::equal(now.lmet.begin() + lm0, now.lmet.begin() + lm0 + M,
                    was.lmet.begin() + lm0)) {
      continue;
    }
    suppress_[rr[k]].push_back(cc[k]);
    counts[rr[k]] -= 1;
    touched[rr[k]] = 1;
  }
  for (uint32_t i = 0; i < V; ++i) {
    if (touched[i]) {
      std::sort(suppress_[i].begin(), suppress_[i].end()); // (the plain rule's columns come first)
    }
  }
}

// applyTopologyChanges of a linksInPlace table: the layout check of the plain
// form is replaced by a match of half-edges by Link identity within each row,
// and a half-edge may change its state as well as its metric.
std::vector<uint32_t> AllNodesRouteTable::applyLinkChanges(const LinkState& ls) {
  const auto tp = std::chrono::steady_clock::now();
  const char* const who = "AllNodesRouteTable::applyTopologyChanges: ";
  // ---- every refusal, before anything is touched
  refuseTopologyChanges(who);
  if (ls.getArea() != area_) {
    throw std::invalid_argument(std::string(who) + "another area");
  }
  LinkState::Engine& eng = ls.engine();
  if (eng.exact) {
    throw std::invalid_argument(std::string(who) + "metric 0 / 64-bit sums need the exact kernel");
  }
  if (eng.names != names_) {
    throw std::invalid_argument(std::string(who) + "nodes changed (build a fresh table)");
  }
  const uint32_t V = (uint32_t)names_.size();
  const size_t E = col_.size();
  {
    std::vector<int32_t> nodeLabel(V, 0);
    for (const auto& [node, db] : ls.getAdjacencyDatabases()) {
      if (db.nodeLabel == 0 || !isMplsLabelValid(db.nodeLabel)) {
        continue;
      }
      if (auto it = ids_.find(node); it != ids_.end()) {
        nodeLabel[it->second] = db.nodeLabel;
      }
    }
    if (nodeLabel != nodeLabel_) {
      throw std::invalid_argument(std::string(who) +
                                  "a node label changed (build a fresh table)");
    }
  }
  // ---- the match: partner[e] = the engine's half-edge of table half-edge e
  // (SPF_MAP_NONE: down now)
  auto same = [](const Link& a, const Link& b, const std::string& node) {
    return a == b && a.getArea() == b.getArea() &&
        a.getIfaceFromNode(node) == b.getIfaceFromNode(node) &&
        a.getNhV4FromNode(node) == b.getNhV4FromNode(node) &&
        a.getNhV6FromNode(node) == b.getNhV6FromNode(node);
  };
  std::vector<uint32_t> partner(E, SPF_MAP_NONE);
  {
    std::unordered_multimap<size_t, uint32_t> byHash;
    for (uint32_t i = 0; i < V; ++i) {
      const uint32_t e0 = row_[i], deg = row_[i + 1] - e0;
      const uint32_t f0 = eng.row[i], degf = eng.row[i + 1] - f0;
      // (a LinkState updated in place keeps its Link objects and the order of
      // a row that lost or gained nothing: position and pointer first)
      bool ident = deg == degf;
      for (uint32_t j = 0; ident && j < deg; ++j) {
        const std::shared_ptr<Link>& now = eng.links[eng.linkId[f0 + j]];
        ident = now == halfLink_[e0 + j] || same(*halfLink_[e0 + j], *now, names_[i]);
      }
      if (ident) {
        for (uint32_t j = 0; j < deg; ++j) {
          partner[e0 + j] = f0 + j;
        }
        continue;
      }
      if (degf > deg) {
        throw std::invalid_argument(std::string(who) +
                                    "a link the table does not hold (build a fresh table)");
      }
      byHash.clear();
      for (uint32_t j = 0; j < deg; ++j) {
        byHash.emplace(halfLink_[e0 + j]->hash, e0 + j);
      }
      for (uint32_t f = f0; f < f0 + degf; ++f) {
        const Link& l = *eng.links[eng.linkId[f]];
        bool found = false;
        auto [lo, hi] = byHash.equal_range(l.hash);
        for (auto it = lo; it != hi; ++it) {
          if (same(*halfLink_[it->second], l, names_[i])) {
            partner[it->second] = f;
            byHash.erase(it); // (a link is one half-edge of the row)
            found = true;
            break;
          }
        }
        if (!found) {
          throw std::invalid_argument(
              std::string(who) +
              "a link the table does not hold, or one that returned with another "
              "identity (build a fresh table)");
        }
      }
    }
  }
  // ---- what changes: state and metric per half-edge
  std::vector<uint32_t> edges, tails;     // half-edges whose state or metric changes
  std::vector<uint8_t> ups;
  std::vector<uint64_t> metrics;
  size_t stateChanges = 0, metricChanges = 0;
  for (uint32_t i = 0; i < V; ++i) {
    for (uint32_t e = row_[i]; e < row_[i + 1]; ++e) {
      const bool wasUp = !isDown(e), isUp = partner[e] != SPF_MAP_NONE;
      if (isUp != (partner[rev_[e]] != SPF_MAP_NONE)) {
        throw std::invalid_argument(std::string(who) +
                                    "the two halves of a link would end in different states");
      }
      if (isUp && eng.col[partner[e]] != col_[e]) {
        throw std::invalid_argument(std::string(who) + "a link changed its identity");
      }
      // (a down half-edge keeps its last metric: never relaxed, but the engine
      // wants a positive one)
      const uint64_t m = isUp ? eng.metric[partner[e]] : metric_[e];
      if (wasUp == isUp && (!isUp || m == metric_[e])) {
        continue;
      }
      if (m == 0 || m > 0x7FFFFFFFull) {
        throw std::invalid_argument(std::string(who) +
                                    "a metric outside the in-place range (0 or above 2^31 - 1)");
      }
      edges.push_back(e);
      ups.push_back(isUp ? 1 : 0);
      metrics.push_back(m);
      stateChanges += wasUp != isUp;
      metricChanges += wasUp && isUp;
      if (tails.empty() || tails.back() != i) {
        tails.push_back(i);
      }
    }
  }
  const std::vector<uint8_t> ovNew(eng.overloaded.begin(), eng.overloaded.end());
  const bool drained = ovNew != overloaded_;
  // ---- edge deltas: the table's up half-edges before the call against the
  // engine's CSR now (a multiset difference per tail: the layouts need not
  // agree).  They only choose rows: not needed when every row is listed.
  uint32_t nd = 0;
  std::vector<spf_edge_delta> deltas(drained ? 0 : stateChanges + 2 * metricChanges);
  if (!deltas.empty()) {
    std::vector<uint32_t> rowUp(V + 1, 0), colUp;
    std::vector<uint64_t> metricUp;
    colUp.reserve(E);
    metricUp.reserve(E);
    for (uint32_t i = 0; i < V; ++i) {
      for (uint32_t e = row_[i]; e < row_[i + 1]; ++e) {
        if (!isDown(e)) {
          colUp.push_back(col_[e]);
          metricUp.push_back(metric_[e]);
        }
      }
      rowUp[i + 1] = (uint32_t)colUp.size();
    }
    spf_graph_desc da{}, db{};
    da.num_nodes = db.num_nodes = V;
    da.num_edges = (uint32_t)colUp.size();
    da.row_ptr = rowUp.data();
    da.col = colUp.data();
    da.metric = metricUp.data();
    da.node_overloaded = overloaded_.data();
    db.num_edges = (uint32_t)eng.col.size();
    db.row_ptr = eng.row.data();
    db.col = eng.col.data();
    db.metric = eng.metric.data();
    db.node_overloaded = ovNew.data();
    da.device = db.device = getSpfDevice();
    if (int s = spf_graph_diff(&da, &db, deltas.data(), (uint32_t)deltas.size(), &nd);
        s != SPF_OK || nd > deltas.size()) {
      tableFailure("spf_graph_diff", s);
    }
  }
  // ---- the rows: every row when an overload bit flipped, else the screen's
  // on the resident rows (before the graph is patched), closed for LFA
  std::vector<uint32_t> rows;
  std::vector<uint32_t> src(V);
  for (uint32_t i = 0; i < V; ++i) {
    src[i] = i;
  }
  if (!drained && !edges.empty()) {
    std::vector<uint8_t> affected(V, 0);
    if (nd) {
      void *dist = nullptr, *nh = nullptr;
      uint32_t eb = 0;
      uint64_t nhWords = 0;
      if (int s = spf_query_device_rows(query_.get(), &dist, &eb, &nh, &nhWords);
          s != SPF_OK || eb != 4) {
        tableFailure("spf_query_device_rows", s);
      }
      if (int s = spf_table_screen(graph_.get(), (const uint32_t*)dist,
                                   spf_query_row_stride(query_.get()), V, src.data(),
                                   deltas.data(), nd, affected.data());
          s != SPF_OK) {
        tableFailure("spf_table_screen", s);
      }
    }
    if (nd != deltas.size()) {
      // parallel links that exchanged metrics (or states) cancel out of the
      // multiset deltas, yet which of them is tight is a link bit of their
      // tail's cells
      for (const uint32_t t : tails) {
        affected[t] = 1;
      }
    }
    // (col_ holds the heads of down half-edges too: a row next to one is
    // listed at worst once too often)
    rows = routeRefreshRowList(affected, row_, col_, tails, lfa_);
  }
  std::vector<uint32_t> counts(V, 0);
  spf_query* q = query_.get();
  std::unique_ptr<spf_query, QueryDeleter> fresh;
  if (drained || !edges.empty()) {
    if (stateChanges) {
      // every check of spf_graph_set_edges comes before its first write: a
      // refusal (a metric the packed edge words cannot hold) still leaves the
      // table as it was
      if (int s = spf_graph_set_edges(graph_.get(), (uint32_t)edges.size(), edges.data(),
                                      ups.data(), metrics.data());
          s == SPF_E_UNSUPPORTED) {
        throw std::invalid_argument(std::string(who) + spf_last_error_detail());
      } else if (s != SPF_OK) {
        tableFailure("spf_graph_set_edges", s);
      }
    } else if (!edges.empty()) {
      if (int s = spf_graph_patch_metrics(graph_.get(), (uint32_t)edges.size(), edges.data(),
                                          metrics.data());
          s != SPF_OK) {
        tableFailure("spf_graph_patch_metrics", s);
      }
    }
    // ---- from here on a failure leaves the table unusable
    if (drained) {
      if (int s = spf_graph_set_transit(graph_.get(), ovNew.data()); s != SPF_OK) {
        tableFailure("spf_graph_set_transit", s);
      }
    }
    spf_query_desc qd{};
    qd.num_queries = V;
    qd.sources = src.data();
    qd.flags = SPF_F_NEXTHOPS;
    spf_query* nq = nullptr;
    if (int s = spf_query_create(graph_.get(), &qd, &nq); s != SPF_OK) {
      tableFailure("spf_query_create", s);
    }
    fresh.reset(nq);
    if (int s = spf_query_run(nq); s != SPF_OK) {
      tableFailure("spf_query_run", s);
    }
    q = nq;
  }
  // (nothing moved on the graph: an all-clear bitmap over the table's own query)
  refreshListedRows(q, drained, rows, counts);
  if (fresh) {
    query_ = std::move(fresh); // (the old query goes: the table is bound to the new one)
    if (int s = spf_query_elapsed_ms(query_.get(), &spfMs_); s != SPF_OK) {
      tableFailure("elapsed", s);
    }
  } else {
    spfMs_ = 0;
  }
  if (int s = spf_route_table_refresh_elapsed_ms(table_.get(), &refreshMs_); s != SPF_OK) {
    tableFailure("spf_route_table_refresh_elapsed_ms", s);
  }
  refreshRows_ = drained ? V : rows.size();
  // ---- a link that went down or came back can move `best` (the smallest
  // REACHABLE announcer) between announcers with equal PrefixEntries: the cell
  // changed, the route did not.  Such cells leave this call's delta.
  // (Selected columns have a rule of their own: suppressSelectedBest below.)
  suppress_.assign(V, {});
  std::vector<uint32_t> risk; // Open/R columns where two announcers share an entry
  for (size_t c = 0; stateChanges && c < numCols(); ++c) {
    if (!isUni(c) || isFree(c) || columnKind(c) != 0) {
      continue;
    }
    const auto& as = annsAt(c);
    bool twin = false;
    for (size_t x = 0; !twin && x < as.size(); ++x) {
      for (size_t y = x + 1; !twin && y < as.size(); ++y) {
        twin = as[x].entry == as[y].entry;
      }
    }
    if (twin) {
      risk.push_back((uint32_t)c);
    }
  }
  if (!risk.empty()) {
    std::vector<uint32_t> rr, cc;
    std::vector<uint64_t> bits((numCols() + 63) / 64);
    uint64_t nl = 0, nm = 0;
    for (uint32_t i = 0; i < V; ++i) {
      if (!counts[i]) {
        continue;
      }
      if (int s = spf_route_table_changed(table_.get(), i, bits.data()); s != SPF_OK) {
        tableFailure("spf_route_table_changed", s);
      }
      const uint64_t deg = row_[i + 1] - row_[i];
      for (const uint32_t c : risk) {
        if ((bits[c / 64] >> (c % 64)) & 1) {
          rr.push_back(i);
          cc.push_back(c);
          nl += (deg + 63) / 64;
          nm += lfa_ ? deg : 0;
        }
      }
    }
    if (!rr.empty()) {
      struct Cells {
        std::vector<uint32_t> metric, best, lmet;
        std::vector<uint64_t> links;
      };
      auto read = [&](decltype(&spf_route_table_fetch_cells) fetch, const char* what) {
        Cells z;
        z.metric.resize(rr.size());
        z.best.resize(rr.size());
        z.links.resize(std::max<uint64_t>(nl, 1));
        z.lmet.resize(std::max<uint64_t>(nm, 1));
        if (int s = fetch(table_.get(), rr.size(), rr.data(), cc.data(), z.metric.data(),
                          z.best.data(), z.links.data(), lfa_ ? z.lmet.data() : nullptr);
            s != SPF_OK) {
          tableFailure(what, s);
        }
        return z;
      };
      const Cells now = read(spf_route_table_fetch_cells, "spf_route_table_fetch_cells");
      const Cells was = read(spf_route_table_fetch_cells_prev, "spf_route_table_fetch_cells_prev");
      auto entryOf = [&](uint32_t c, uint32_t id) -> const thrift::PrefixEntry* {
        for (const auto& a : annsAt(c)) {
          if (a.id == id) {
            return &a.entry;
          }
        }
        return nullptr;
      };
      uint64_t lw = 0, lm = 0;
      for (size_t k = 0; k < rr.size(); ++k) {
        const uint64_t deg = row_[rr[k] + 1] - row_[rr[k]], W = (deg + 63) / 64, M = lfa_ ? deg : 0;
        const uint64_t lw0 = lw, lm0 = lm;
        lw += W;
        lm += M;
        if (was.metric[k] == 0xFFFFFFFFu || now.metric[k] == 0xFFFFFFFFu ||
            was.best[k] == now.best[k]) {
          continue;
        }
        const auto* oe = entryOf(cc[k], was.best[k]);
        const auto* ne = entryOf(cc[k], now.best[k]);
        if (!oe || !ne || !(*oe == *ne)) {
          continue;
        }
        // (LFA: the metric word is no part of the route, see diff())
        if ((!lfa_ && was.metric[k] != now.metric[k]) ||
            !std::equal(now.links.begin() + lw0, now.links.begin() + lw0 + W,
                        was.links.begin() + lw0) ||
            !std::equal(now.lmet.begin() + lm0, now.lmet.begin() + lm0 + M,
                        was.lmet.begin() + lm0)) {
          continue;
        }
        suppress_[rr[k]].push_back(cc[k]); // (rows and columns ascending: sorted)
        counts[rr[k]] -= 1;
      }
    }
  }
  suppressSelectedBest(counts);
  // ---- the host's view: states, metrics, drain bits, links, adjacency labels
  if (stateChanges && down_.empty()) {
    down_.assign(E, 0);
  }
  for (size_t k = 0; k < edges.size(); ++k) {
    metric_[edges[k]] = metrics[k];
    if (!down_.empty()) {
      down_[edges[k]] = !ups[k];
    }
  }
  downLinks_ = (size_t)std::count(down_.begin(), down_.end(), (uint8_t)1) / 2;
  overloaded_ = ovNew;
  for (size_t e = 0; e < E; ++e) {
    // (a down half-edge keeps its Link: previous cells may name it)
    if (partner[e] != SPF_MAP_NONE) {
      halfLink_[e] = eng.links[eng.linkId[partner[e]]];
    }
  }
  prevAdjLabels_ = std::move(adjLabels_);
  adjLabels_.clear();
  collectAdjLabels(ls);
  diffed_ = true;
  mapped_ = false;
  patchDelta_ = false;
  topoDelta_ = true;
  older_ = nullptr;
  goneCols_.clear();
  goneNew_.clear();
  rowOf_.resize(V);
  for (uint32_t i = 0; i < V; ++i) {
    rowOf_[i] = i;
  }
  Counters::add("decision.route_table_refresh_us", usSince(tp));
  return counts;
}

std::vector<uint32_t> AllNodesRouteTable::applyTopologyChanges(const LinkState& ls) {
  if (linksInPlace_) {
    return applyLinkChanges(ls);
  }
  const auto tp = std::chrono::steady_clock::now();
  // ---- every refusal, before anything is touched
  refuseTopologyChanges("AllNodesRouteTable::applyTopologyChanges: ");
  if (ls.getArea() != area_) {
    throw std::invalid_argument("AllNodesRouteTable::applyTopologyChanges: another area");
  }
  LinkState::Engine& eng = ls.engine();
  if (eng.exact) {
    throw std::invalid_argument(
        "AllNodesRouteTable::applyTopologyChanges: metric 0 / 64-bit sums need the exact kernel");
  }
  if (eng.names != names_ || eng.row != row_ || eng.col != col_ || eng.rev != rev_ ||
      eng.linkId != linkId_) {
    throw std::invalid_argument(
        "AllNodesRouteTable::applyTopologyChanges: nodes or links changed (build a fresh table)");
  }
  const uint32_t V = (uint32_t)names_.size();
  const size_t E = col_.size();
  // (a LinkState updated in place keeps its Link objects: the usual case is
  // pointer equality, and only other objects are compared and taken over)
  std::vector<std::pair<uint32_t, std::shared_ptr<Link>>> moved;
  for (uint32_t i = 0; i < V; ++i) {
    for (uint32_t e = row_[i]; e < row_[i + 1]; ++e) {
      const std::shared_ptr<Link>& now = eng.links[eng.linkId[e]];
      if (now == halfLink_[e]) {
        continue;
      }
      moved.emplace_back(e, now);
      const Link& a = *halfLink_[e];
      const Link& b = *now;
      const std::string& node = names_[i];
      if (!(a == b && a.getArea() == b.getArea() &&
            a.getIfaceFromNode(node) == b.getIfaceFromNode(node) &&
            a.getNhV4FromNode(node) == b.getNhV4FromNode(node) &&
            a.getNhV6FromNode(node) == b.getNhV6FromNode(node))) {
        throw std::invalid_argument(
            "AllNodesRouteTable::applyTopologyChanges: a link changed its identity");
      }
    }
  }
  {
    std::vector<int32_t> nodeLabel(V, 0);
    for (const auto& [node, db] : ls.getAdjacencyDatabases()) {
      if (db.nodeLabel == 0 || !isMplsLabelValid(db.nodeLabel)) {
        continue;
      }
      if (auto it = ids_.find(node); it != ids_.end()) {
        nodeLabel[it->second] = db.nodeLabel;
      }
    }
    if (nodeLabel != nodeLabel_) {
      throw std::invalid_argument(
          "AllNodesRouteTable::applyTopologyChanges: a node label changed (build a fresh table)");
    }
  }
  // ---- edge deltas between the two CSR snapshots, changed half-edges
  auto desc = [&](const std::vector<uint64_t>& metric, const std::vector<uint8_t>& ov) {
    spf_graph_desc d{};
    d.num_nodes = V;
    d.num_edges = (uint32_t)E;
    d.row_ptr = row_.data();
    d.col = col_.data();
    d.metric = metric.data();
    d.link_id = linkId_.data();
    d.rev = rev_.data();
    d.node_overloaded = ov.data();
    d.num_links = numLinks_;
    d.device = getSpfDevice();
    return d;
  };
  const std::vector<uint8_t> ovNew(eng.overloaded.begin(), eng.overloaded.end());
  std::vector<uint32_t> edges, tails;
  std::vector<uint64_t> metrics;
  for (uint32_t i = 0; i < V; ++i) {
    for (uint32_t e = row_[i]; e < row_[i + 1]; ++e) {
      if (metric_[e] != eng.metric[e]) {
        edges.push_back(e);
        metrics.push_back(eng.metric[e]);
        if (tails.empty() || tails.back() != i) {
          tails.push_back(i);
        }
      }
    }
  }
  const bool drained = ovNew != overloaded_;
  // (the deltas only choose rows: not needed when every row is listed, none
  // without a changed metric; a changed half-edge gives at most two)
  uint32_t nd = 0;
  std::vector<spf_edge_delta> deltas(drained ? 0 : 2 * edges.size());
  if (!deltas.empty()) {
    const spf_graph_desc da = desc(metric_, overloaded_), db = desc(eng.metric, ovNew);
    if (int s = spf_graph_diff(&da, &db, deltas.data(), (uint32_t)deltas.size(), &nd);
        s != SPF_OK || nd > deltas.size()) {
      tableFailure("spf_graph_diff", s);
    }
  }
  // ---- the rows: every row when an overload bit flipped, else the screen's
  // on the resident rows (before the graph is patched), closed for LFA
  std::vector<uint32_t> rows;
  std::vector<uint32_t> src(V);
  for (uint32_t i = 0; i < V; ++i) {
    src[i] = i;
  }
  if (!drained && !edges.empty()) {
    std::vector<uint8_t> affected(V, 0);
    if (nd) {
      void *dist = nullptr, *nh = nullptr;
      uint32_t eb = 0;
      uint64_t nhWords = 0;
      if (int s = spf_query_device_rows(query_.get(), &dist, &eb, &nh, &nhWords);
          s != SPF_OK || eb != 4) {
        tableFailure("spf_query_device_rows", s);
      }
      if (int s = spf_table_screen(graph_.get(), (const uint32_t*)dist,
                                   spf_query_row_stride(query_.get()), V, src.data(),
                                   deltas.data(), nd, affected.data());
          s != SPF_OK) {
        tableFailure("spf_table_screen", s);
      }
    }
    if (nd != 2 * edges.size()) {
      // parallel links that exchanged metrics cancel out of the multiset
      // deltas, yet which of them is tight is a link bit of their tail's cells
      for (const uint32_t t : tails) {
        affected[t] = 1;
      }
    }
    rows = routeRefreshRowList(affected, row_, col_, tails, lfa_);
  }
  std::vector<uint32_t> counts(V, 0);
  spf_query* q = query_.get();
  std::unique_ptr<spf_query, QueryDeleter> fresh;
  if (drained || !edges.empty()) {
    // ---- from here on a failure leaves the table unusable
    if (!edges.empty()) {
      if (int s = spf_graph_patch_metrics(graph_.get(), (uint32_t)edges.size(), edges.data(),
                                          metrics.data());
          s != SPF_OK) {
        tableFailure("spf_graph_patch_metrics", s);
      }
    }
    if (drained) {
      if (int s = spf_graph_set_transit(graph_.get(), ovNew.data()); s != SPF_OK) {
        tableFailure("spf_graph_set_transit", s);
      }
    }
    spf_query_desc qd{};
    qd.num_queries = V;
    qd.sources = src.data();
    qd.flags = SPF_F_NEXTHOPS;
    spf_query* nq = nullptr;
    if (int s = spf_query_create(graph_.get(), &qd, &nq); s != SPF_OK) {
      tableFailure("spf_query_create", s);
    }
    fresh.reset(nq);
    if (int s = spf_query_run(nq); s != SPF_OK) {
      tableFailure("spf_query_run", s);
    }
    q = nq;
  }
  // (nothing moved on the graph: an all-clear bitmap over the table's own query)
  refreshListedRows(q, drained, rows, counts);
  if (fresh) {
    query_ = std::move(fresh); // (the old query goes: the table is bound to the new one)
    if (int s = spf_query_elapsed_ms(query_.get(), &spfMs_); s != SPF_OK) {
      tableFailure("elapsed", s);
    }
  } else {
    spfMs_ = 0;
  }
  if (int s = spf_route_table_refresh_elapsed_ms(table_.get(), &refreshMs_); s != SPF_OK) {
    tableFailure("spf_route_table_refresh_elapsed_ms", s);
  }
  refreshRows_ = drained ? V : rows.size();
  // (metrics and drains cut no announcer off: `best` of an Open/R column stays;
  // the best candidate of a selected column follows the distances)
  suppress_.assign(V, {});
  suppressSelectedBest(counts);
  // ---- the host's view: metrics, drain bits, links, adjacency labels
  metric_ = eng.metric;
  overloaded_ = ovNew;
  for (auto& [e, link] : moved) {
    halfLink_[e] = std::move(link);
  }
  prevAdjLabels_ = std::move(adjLabels_);
  adjLabels_.clear();
  collectAdjLabels(ls);
  diffed_ = true;
  mapped_ = false;
  patchDelta_ = false;
  topoDelta_ = true;
  older_ = nullptr;
  goneCols_.clear();
  goneNew_.clear();
  rowOf_.resize(V);
  for (uint32_t i = 0; i < V; ++i) {
    rowOf_[i] = i;
  }
  Counters::add("decision.route_table_refresh_us", usSince(tp));
  return counts;
}

std::pair<uint32_t, uint32_t> AllNodesRouteTable::changedSplit(const std::string& node) const {
  if (!diffed_) {
    throw std::logic_error("AllNodesRouteTable::changedSplit: no diff has run");
  }
  auto it = ids_.find(node);
  const size_t C = numCols();
  if (it == ids_.end() || (!C && goneCols_.empty())) {
    return {0, 0};
  }
  std::vector<uint64_t> bits((C + 63) / 64);
  if (C) {
    if (int s = spf_route_table_changed(table_.get(), it->second, bits.data()); s != SPF_OK) {
      tableFailure("spf_route_table_changed", s);
    }
  }
  uint32_t uni = 0, lab = 0;
  forEachSetBit(bits.data(), bits.size(), [&](size_t p) { (isUni(p) ? uni : lab) += 1; });
  if (patchDelta_ || topoDelta_) {
    uni -= (uint32_t)suppress_[it->second].size();
  }
  if (!goneCols_.empty()) {
    // deleted columns of the older table
    std::vector<uint64_t> gbits((goneCols_.size() + 63) / 64);
    if (int s = spf_route_table_changed_gone(table_.get(), it->second, gbits.data());
        s != SPF_OK) {
      tableFailure("spf_route_table_changed_gone", s);
    }
    forEachSetBit(gbits.data(), gbits.size(), [&](size_t g) {
      const uint32_t p = goneNew_[g];
      if (p != SPF_MAP_NONE && ((bits[p / 64] >> (p % 64)) & 1)) {
        return; // the column changed its kind: counted as the update already
      }
      (older_->isUni(goneCols_[g]) ? uni : lab) += 1;
    });
  }
  return {uni, lab};
}

std::vector<int32_t> AllNodesRouteTable::labelCandidates(
    uint32_t i, const uint32_t* cols, size_t n, const uint32_t* gone, size_t ng) const {
  if (patchDelta_) {
    return {}; // a prefix change moves no label column and no adjacency label
  }
  const uint32_t ia = rowOf_[i];
  const bool hasOld = ia != SPF_MAP_NONE;
  const size_t P = prefixes_.size();
  std::set<int32_t> labels;
  for (const AdjLabel& a : adjLabels_[i]) {
    labels.insert(a.label);
  }
  if (topoDelta_) {
    // the older side is this table before the call: same label columns, the
    // previous adjacency labels, nothing gone
    for (const AdjLabel& a : prevAdjLabels_[i]) {
      labels.insert(a.label);
    }
    for (size_t k = 0; k < n; ++k) {
      if (!isUni(cols[k])) {
        labels.insert(owners_[cols[k] - P].label);
      }
    }
    return {labels.begin(), labels.end()};
  }
  const size_t Pa = older_->prefixes_.size();
  if (hasOld) {
    for (const AdjLabel& a : older_->adjLabels_[ia]) {
      labels.insert(a.label);
    }
  }
  if (mapped_) {
    // the node's own label: POP_AND_LOOKUP has no cell behind it
    if (nodeLabel_[i]) {
      labels.insert(nodeLabel_[i]);
    }
    if (hasOld && older_->nodeLabel_[ia]) {
      labels.insert(older_->nodeLabel_[ia]);
    }
  }
  for (size_t k = 0; k < ng; ++k) {
    const uint32_t c = goneCols_[gone[k]];
    if (!older_->isUni(c)) {
      labels.insert(older_->owners_[c - Pa].label);
    }
  }
  for (size_t k = 0; k < n; ++k) {
    if (!isUni(cols[k])) {
      labels.insert(owners_[cols[k] - P].label);
    }
  }
  return {labels.begin(), labels.end()};
}

void AllNodesRouteTable::unicastDelta(
    uint32_t i, const Row& r, const uint32_t* cols, size_t n, const uint32_t* gone, size_t ng,
    DecisionRouteUpdate& u) const {
  // (ng == 0 after applyPrefixChanges, where older_ is null)
  for (size_t k = 0; k < ng; ++k) {
    const uint32_t c = goneCols_[gone[k]];
    // (a column that changed its kind and still has a route here: the update
    // below replaces the older route)
    if (older_->isUni(c) && !std::binary_search(cols, cols + n, goneNew_[gone[k]])) {
      u.unicastRoutesToDelete.push_back(older_->prefixAt(c));
    }
  }
  for (size_t k = 0; k < n; ++k) {
    const size_t p = cols[k];
    if (!isUni(p)) {
      continue; // a label column: among the MPLS candidates
    }
    if (r.metricOf(p) == 0xFFFFFFFFu) {
      u.unicastRoutesToDelete.push_back(prefixAt(p));
    } else {
      u.unicastRoutesToUpdate.push_back(materialise(names_[i], i, r, p));
    }
  }
}

void AllNodesRouteTable::mplsDelta(
    uint32_t i, const Row& r, uint32_t ia, const Row& o, const std::vector<int32_t>& labels,
    DecisionRouteUpdate& u) const {
  for (const int32_t label : labels) {
    auto ne = mplsEntry(i, r, label);
    auto oe = topoDelta_ ? mplsEntryWith(i, o, label, prevAdjLabels_[i])
        : ia != SPF_MAP_NONE ? older_->mplsEntry(ia, o, label)
                             : std::nullopt;
    if (ne && (!oe || !(*oe == *ne))) {
      u.mplsRoutesToUpdate.push_back(std::move(*ne));
    } else if (!ne && oe) {
      u.mplsRoutesToDelete.push_back(label);
    }
  }
}

DecisionRouteUpdate AllNodesRouteTable::delta(const std::string& node) const {
  DecisionRouteUpdate u;
  auto it = ids_.find(node);
  if (!diffed_) {
    throw std::logic_error("AllNodesRouteTable::delta: no diff has run");
  }
  if (it == ids_.end()) {
    return u;
  }
  const uint32_t i = it->second;
  const size_t C = numCols();
  // the bitmaps first: changed columns and, after a mapped diff, the set
  // bits of the gone bitmap (deleted columns of the older table)
  std::vector<uint32_t> cols, gone;
  if (C) {
    std::vector<uint64_t> bits((C + 63) / 64);
    if (int s = spf_route_table_changed(table_.get(), i, bits.data()); s != SPF_OK) {
      tableFailure("spf_route_table_changed", s);
    }
    forEachSetBit(bits.data(), bits.size(), [&](size_t p) {
      if (!suppressed(i, (uint32_t)p)) {
        cols.push_back((uint32_t)p);
      }
    });
  }
  if (mapped_ && !goneCols_.empty()) {
    std::vector<uint64_t> gbits((goneCols_.size() + 63) / 64);
    if (int s = spf_route_table_changed_gone(table_.get(), i, gbits.data()); s != SPF_OK) {
      tableFailure("spf_route_table_changed_gone", s);
    }
    forEachSetBit(gbits.data(), gbits.size(), [&](size_t g) { gone.push_back((uint32_t)g); });
  }
  const std::vector<int32_t> labels =
      labelCandidates(i, cols.data(), cols.size(), gone.data(), gone.size());
  // then whole rows, where something reads them: this node's, and for MPLS
  // candidates its row in the older table (none: every route here is new)
  const Row r = C && (!cols.empty() || !labels.empty()) ? fetchRow(i) : Row{};
  unicastDelta(i, r, cols.data(), cols.size(), gone.data(), gone.size(), u);
  if (!labels.empty()) {
    const uint32_t ia = rowOf_[i];
    if (topoDelta_) {
      mplsDelta(i, r, ia, C ? fetchPrevRow(i) : Row{}, labels, u);
      return u;
    }
    const size_t Ca = older_->numCols();
    const Row o = ia != SPF_MAP_NONE && Ca ? older_->fetchRow(ia) : Row{};
    mplsDelta(i, r, ia, o, labels, u);
  }
  return u;
}

uint64_t AllNodesRouteTable::deltaFetchBytes(const std::string& node) const {
  auto it = ids_.find(node);
  if (!diffed_ || it == ids_.end()) {
    return 0;
  }
  const uint32_t i = it->second;
  auto rowBytes = [](const AllNodesRouteTable& t, uint32_t r) {
    const uint64_t C = t.numCols();
    const uint64_t deg = t.row_[r + 1] - t.row_[r];
    // (tables with selected columns: the row's igp and winners words too)
    return C * (8 + ((deg + 63) / 64) * 8 + (t.lfa_ ? deg * 4 : 0)) + (uint64_t)t.devSel_ * 8;
  };
  const uint64_t C = numCols();
  uint64_t b = ((C + 63) / 64) * 8 + rowBytes(*this, i);
  if (mapped_ && !goneCols_.empty()) {
    b += ((goneCols_.size() + 63) / 64) * 8;
  }
  if (older_ && rowOf_[i] != SPF_MAP_NONE) {
    b += rowBytes(*older_, rowOf_[i]);
  }
  return b;
}

std::vector<DecisionRouteUpdate> AllNodesRouteTable::deltas() const {
  if (!diffed_) {
    throw std::logic_error("AllNodesRouteTable::deltas: no diff has run");
  }
  using Clock = std::chrono::steady_clock;
  auto us = [](Clock::time_point a, Clock::time_point b) {
    return std::chrono::duration<double, std::micro>(b - a).count();
  };
  const auto t0 = Clock::now();
  const uint32_t V = (uint32_t)names_.size();
  std::vector<DecisionRouteUpdate> out(V);
  DeltasStats st;

  // ---- the changed cells of every row, compacted on the device
  spf_route_delta_sizes z{};
  if (int s = spf_route_table_delta_pack(table_.get(), &z); s != SPF_OK) {
    tableFailure("spf_route_table_delta_pack", s);
  }
  const auto t1 = Clock::now();
  std::vector<uint64_t> cellOff((size_t)V + 1), goneOff((size_t)V + 1);
  std::vector<uint32_t> col(z.cells), metric(z.cells), best(z.cells), gone(z.gone);
  std::vector<uint64_t> links(z.link_words);
  std::vector<uint32_t> lmet(z.link_metrics);
  if (int s = spf_route_table_delta_fetch(
          table_.get(), cellOff.data(), col.data(), metric.data(), best.data(), links.data(),
          lfa_ ? lmet.data() : nullptr, goneOff.data(), gone.data());
      s != SPF_OK) {
    tableFailure("spf_route_table_delta_fetch", s);
  }
  // selected columns: the igp lane of the packed list (bestNexthop.metric)
  std::vector<uint32_t> igp(devSel_ ? z.cells : 0);
  if (devSel_) {
    if (int s = spf_route_table_delta_fetch_igp(table_.get(), igp.data()); s != SPF_OK) {
      tableFailure("spf_route_table_delta_fetch_igp", s);
    }
  }
  const auto t2 = Clock::now();
  auto degOf = [](const AllNodesRouteTable& t, uint32_t r) {
    return (size_t)(t.row_[r + 1] - t.row_[r]);
  };
  // link-word and link-metric base of every row's cells in the packed list
  std::vector<uint64_t> lwBase((size_t)V + 1, 0), lmBase((size_t)V + 1, 0);
  for (uint32_t i = 0; i < V; ++i) {
    const uint64_t n = cellOff[i + 1] - cellOff[i], deg = degOf(*this, i);
    lwBase[i + 1] = lwBase[i] + n * ((deg + 63) / 64);
    lmBase[i + 1] = lmBase[i] + (lfa_ ? n * deg : 0);
  }

  // ---- MPLS candidates of every node (the labels delta() compares) and the
  // cells mplsEntry reads for them: every column of the label, in both tables
  // (after applyTopologyChanges the older side is this table's previous cells)
  const AllNodesRouteTable* const old = topoDelta_ ? this : older_;
  std::vector<std::vector<int32_t>> labelsOf(V);
  std::vector<std::vector<uint32_t>> colsN(V), colsO(V);
  const unsigned threads = hostThreads(V, 64);
  parallelFor(V, threads, [&](size_t n, unsigned) {
    const uint32_t i = (uint32_t)n;
    const bool hasOld = rowOf_[i] != SPF_MAP_NONE;
    labelsOf[i] = labelCandidates(
        i, col.data() + cellOff[i], (size_t)(cellOff[i + 1] - cellOff[i]), gone.data() + goneOff[i],
        (size_t)(goneOff[i + 1] - goneOff[i]));
    for (const int32_t label : labelsOf[i]) {
      if (auto lc = labelCols_.find(label); lc != labelCols_.end()) {
        colsN[i].insert(colsN[i].end(), lc->second.begin(), lc->second.end());
      }
      if (hasOld) {
        if (auto lc = old->labelCols_.find(label); lc != old->labelCols_.end()) {
          colsO[i].insert(colsO[i].end(), lc->second.begin(), lc->second.end());
        }
      }
    }
    std::sort(colsN[i].begin(), colsN[i].end());
    std::sort(colsO[i].begin(), colsO[i].end());
  });

  // ---- one sparse read per table
  struct Cells {
    std::vector<uint64_t> off, lwPos, lmPos; // per node: first cell, link word, link metric
    std::vector<uint32_t> rows, cols, metric, best, lmet;
    std::vector<uint64_t> links;
  };
  auto gather = [&](const AllNodesRouteTable& t, const std::vector<std::vector<uint32_t>>& want,
                    bool older) {
    Cells c;
    c.off.assign((size_t)V + 1, 0);
    c.lwPos.assign((size_t)V + 1, 0);
    c.lmPos.assign((size_t)V + 1, 0);
    for (uint32_t i = 0; i < V; ++i) {
      const uint64_t n = want[i].size();
      const uint32_t r = older ? rowOf_[i] : i;
      const uint64_t deg = n ? degOf(t, r) : 0;
      c.off[i + 1] = c.off[i] + n;
      c.lwPos[i + 1] = c.lwPos[i] + n * ((deg + 63) / 64);
      c.lmPos[i + 1] = c.lmPos[i] + (lfa_ ? n * deg : 0);
      c.rows.insert(c.rows.end(), n, r);
      c.cols.insert(c.cols.end(), want[i].begin(), want[i].end());
    }
    const uint64_t n = c.rows.size();
    c.metric.resize(n);
    c.best.resize(n);
    c.links.resize(c.lwPos[V]);
    c.lmet.resize(c.lmPos[V]);
    const auto fetch = older && topoDelta_ ? spf_route_table_fetch_cells_prev
                                           : spf_route_table_fetch_cells;
    if (int s = fetch(t.table_.get(), n, c.rows.data(), c.cols.data(), c.metric.data(),
                      c.best.data(), c.links.data(), lfa_ ? c.lmet.data() : nullptr);
        s != SPF_OK) {
      tableFailure("spf_route_table_fetch_cells", s);
    }
    return c;
  };
  const Cells cn = gather(*this, colsN, false);
  const Cells co = old ? gather(*old, colsO, true) : Cells{}; // (null: no candidates)
  const auto t3 = Clock::now();

  // a sparse Row over cells [k0, k1) of one node in a cell list
  auto view = [&](const AllNodesRouteTable& t, uint32_t r, const uint32_t* cols,
                  const uint32_t* metric, const uint32_t* best, size_t n, const uint64_t* links,
                  const uint32_t* lmet, const uint32_t* igp = nullptr) {
    Row v;
    v.sparse = true;
    v.deg = degOf(t, r);
    v.W = (v.deg + 63) / 64;
    v.cols.assign(cols, cols + n);
    v.metric.assign(metric, metric + n);
    v.best.assign(best, best + n);
    v.links.assign(links, links + n * v.W);
    if (lfa_) {
      v.lmet.assign(lmet, lmet + n * v.deg);
    }
    if (igp) {
      v.igp.assign(igp, igp + n);
    }
    return v;
  };

  // ---- assembly, node by node on the worker pool
  parallelFor(V, threads, [&](size_t n, unsigned) {
    const uint32_t i = (uint32_t)n;
    DecisionRouteUpdate& u = out[i];
    const uint32_t ia = rowOf_[i];
    const bool hasOld = ia != SPF_MAP_NONE;
    const uint64_t k0 = cellOff[i], k1 = cellOff[i + 1];
    const Row r = k1 > k0
        ? view(*this, i, col.data() + k0, metric.data() + k0, best.data() + k0, (size_t)(k1 - k0),
               links.data() + lwBase[i], lmet.data() + lmBase[i],
               devSel_ ? igp.data() + k0 : nullptr)
        : Row{};
    if ((patchDelta_ || topoDelta_) && !suppress_[i].empty()) {
      std::vector<uint32_t> keep;
      for (uint64_t k = k0; k < k1; ++k) {
        if (!suppressed(i, col[k])) {
          keep.push_back(col[k]);
        }
      }
      unicastDelta(i, r, keep.data(), keep.size(), nullptr, 0, u);
    } else {
      unicastDelta(i, r, col.data() + k0, (size_t)(k1 - k0), gone.data() + goneOff[i],
                   (size_t)(goneOff[i + 1] - goneOff[i]), u);
    }
    if (labelsOf[i].empty()) {
      return;
    }
    const size_t a0 = cn.off[i], b0 = co.off[i];
    const Row rn = view(*this, i, cn.cols.data() + a0, cn.metric.data() + a0, cn.best.data() + a0,
                        (size_t)(cn.off[i + 1] - a0), cn.links.data() + cn.lwPos[i],
                        cn.lmet.data() + cn.lmPos[i]);
    Row ro;
    if (hasOld) {
      ro = view(*old, ia, co.cols.data() + b0, co.metric.data() + b0, co.best.data() + b0,
                (size_t)(co.off[i + 1] - b0), co.links.data() + co.lwPos[i],
                co.lmet.data() + co.lmPos[i]);
    }
    mplsDelta(i, rn, ia, ro, labelsOf[i], u);
  });
  const auto t4 = Clock::now();

  st.packUs = us(t0, t1);
  st.fetchUs = us(t1, t2);
  st.gatherUs = us(t2, t3);
  st.assembleUs = us(t3, t4);
  st.totalUs = us(t0, t4);
  st.cells = z.cells;
  st.gone = z.gone;
  st.linkWords = z.link_words;
  st.linkMetrics = z.link_metrics;
  st.newerCells = cn.rows.size();
  st.olderCells = co.rows.size();
  // what crossed from the device: the pack's totals, the packed list, and per
  // gathered cell its metric and best, plus the link words and link metrics
  // (tables with selected columns: the igp lane, one more word per cell)
  st.bytes = 32 + 2 * ((uint64_t)V + 1) * 8 + z.cells * (devSel_ ? 16 : 12) + z.link_words * 8 +
      z.link_metrics * 4 + z.gone * 4 + (st.newerCells + st.olderCells) * 8 +
      (cn.links.size() + co.links.size()) * 8 + (cn.lmet.size() + co.lmet.size()) * 4;
  lastDeltas_ = st;
  Counters::add("decision.route_table_deltas_us", (int64_t)st.totalUs);
  Counters::add("decision.route_table_deltas_cells", (int64_t)z.cells);
  return out;
}

AllAreasRouteTable::AllAreasRouteTable(
    const std::unordered_map<std::string, LinkState>& areas, const PrefixState& ps,
    bool enableV4, bool computeLfa, bool bgpDryRun, bool bgpUseIgpMetric, bool prefetchAll,
    bool bgpIgpOnDevice)
    : areas_(areas),
      ps_(ps),
      enableV4_(enableV4),
      lfa_(computeLfa),
      bgpDryRun_(bgpDryRun),
      bgpIgp_(bgpUseIgpMetric) {
  // nodes of every area (hasNode, LinkState.h) -> border nodes (>= 2 areas)
  std::unordered_map<std::string, std::vector<std::string>> areasOf;
  for (const auto& [area, ls] : areas_) {
    for (const auto& [node, _] : ls.getAdjacencyDatabases()) {
      if (ls.hasNode(node)) {
        areasOf[node].push_back(area);
      }
    }
  }
  for (const auto& [node, as] : areasOf) {
    if (as.size() > 1) {
      border_.insert(node);
    } else {
      home_[node] = as.front();
    }
  }
  const bool multi = areas_.size() > 1;
  for (const auto& [area, ls] : areas_) {
    if (ls.engine().exact) {
      continue; // metric 0 / 64-bit sums: this area stays on the host path
    }
    // BGP prefixes join the device table when the selection cannot depend
    // on the node (no IGP cost in the metric vector), or, with
    // bgpIgpOnDevice, as selected columns folded per node on the device
    auto t = std::make_unique<AllNodesRouteTable>(
        ls, ps, enableV4, computeLfa, multi ? &border_ : nullptr,
        (!bgpUseIgpMetric || bgpIgpOnDevice) && std::getenv("OPENR_RT_BGP_HOST") == nullptr,
        bgpDryRun, bgpUseIgpMetric);
    auto& served = served_[area];
    for (const auto& p : t->prefixes()) {
      served.insert(p);
    }
    rest_[area] = served.size() < ps.prefixes().size();
    tables_[area] = std::move(t);
    if (prefetchAll) {
      // the host share then reads resident rows only (one batch per area)
      std::vector<std::string> all;
      for (const auto& [node, as] : areasOf) {
        if (std::find(as.begin(), as.end(), area) != as.end()) {
          all.push_back(node);
        }
      }
      ls.prefetchSpf(all, true);
    }
  }
}

AllAreasRouteTable::~AllAreasRouteTable() = default;

const AllNodesRouteTable* AllAreasRouteTable::areaTable(const std::string& area) const {
  auto it = tables_.find(area);
  return it == tables_.end() ? nullptr : it->second.get();
}

std::optional<DecisionRouteDb> AllAreasRouteTable::routeDb(const std::string& node) const {
  lastTable_ = lastHost_ = 0;
  bool known = false;
  for (const auto& [_, ls] : areas_) {
    known |= ls.hasNode(node);
  }
  if (!known) {
    return std::nullopt;
  }
  SpfSolver solver(node, enableV4_, lfa_, false, bgpDryRun_, bgpIgp_);
  const auto h = home_.find(node);
  const auto t = h == home_.end() ? tables_.end() : tables_.find(h->second);
  if (t == tables_.end()) {
    // border node (or an area the kernel does not take): the host path
    auto db = solver.buildRouteDb(node, areas_, ps_);
    if (db) {
      lastHost_ = db->unicastEntries.size() + db->mplsEntries.size();
    }
    return db;
  }
  const bool single = areas_.size() == 1;
  DecisionRouteDb db;
  db.unicastEntries = t->second->routes(node);
  if (single) {
    db.mplsEntries = t->second->mplsRoutes(node);
  }
  lastTable_ = db.unicastEntries.size() + db.mplsEntries.size();
  if (!single || rest_.at(h->second)) {
    auto part = solver.buildRouteDbPartial(node, areas_, ps_, served_.at(h->second), !single);
    if (part) {
      lastHost_ = part->unicastEntries.size() + (single ? 0 : part->mplsEntries.size());
      for (auto& [p, e] : part->unicastEntries) {
        db.unicastEntries.emplace(p, std::move(e));
      }
      if (!single) {
        db.mplsEntries = std::move(part->mplsEntries);
      }
    }
  }
  return db;
}

} // namespace openr
