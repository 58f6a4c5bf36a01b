// cli_graph.cpp -- the unitig graph of the finished count, for the `cfrk` command: simplify (--unitigs-clip-tips,
// --unitigs-pop-bubbles, --unitigs-pop-bulges, --unitigs-drop-weak), write (--unitigs-out, --unitigs-links, --unitigs-gfa), map reads onto it (--unitigs-map)
// and thread them through it (--unitigs-map-paths, --unitigs-link-support, --unitigs-map-stats); its connected components
// (--unitigs-components, --unitigs-component-tags, --unitigs-min-component-kmers, --unitigs-map-components).
#include "cli_util.h"

namespace {

// The unitigs of the finished result through the host form (a sizes-only call, then arrays of that size) and, on request,
// the links between them, the same way.  The text of a compacted graph is small beside the count's input: one thread formats it.
struct UnitigGraph {
  int64_t nN = 0, nS = 0, n_links = 0;
  std::vector<int8_t> data;
  std::vector<int64_t> start, link_ptr;
  std::vector<int32_t> length;
  std::vector<cfrk_unitig> rec;
  std::vector<cfrk_unitig_link> links;
  // 0, or the exit status (the error reported)
  int fetch(cfrk_ctx *ctx, uint32_t min_count, bool with_links) {
    int rc = sized_call([&] { return cfrk_global_unitigs(ctx, min_count, data.data(), data.size(), start.data(), length.data(), rec.data(), rec.size(), &nN, &nS); },
                        [&] { data.resize((size_t)nN); start.resize((size_t)nS); length.resize((size_t)nS); rec.resize((size_t)nS); });
    if (rc) return die(ctx, rc, "cfrk_global_unitigs");
    return with_links ? fetch_links(ctx, min_count) : 0;
  }
  int fetch_links(cfrk_ctx *ctx, uint32_t min_count) {
    int rc;
    link_ptr.resize((size_t)nS + 1);
    rc = sized_call([&] { return cfrk_global_unitig_links(ctx, min_count, data.data(), start.data(), length.data(), nN, nS, link_ptr.data(), links.data(), links.size(), &n_links); },
                    [&] { links.resize((size_t)n_links); });
    return rc ? die(ctx, rc, "cfrk_global_unitig_links") : 0;
  }
  // --simplify-recompact: the unitigs of this graph without the dropped ones, from the graph itself (this one needs its links)
  int compact_into(cfrk_ctx *ctx, const uint8_t *drop, UnitigGraph *out) const {
    UnitigGraph &n = *out;
    const int rc = sized_call([&] { return cfrk_global_unitigs_compact(ctx, data.data(), start.data(), length.data(), rec.data(), nN, nS, link_ptr.data(),
                                                                        links.data(), n_links, drop, n.data.data(), n.data.size(), n.start.data(),
                                                                        n.length.data(), n.rec.data(), n.rec.size(), nullptr, &n.nN, &n.nS); },
                              [&] { n.data.resize((size_t)n.nN); n.start.resize((size_t)n.nS); n.length.resize((size_t)n.nS); n.rec.resize((size_t)n.nS); });
    return rc ? die(ctx, rc, "cfrk_global_unitigs_compact") : 0;
  }
};

}  // namespace

// --unitigs-clip-tips, --unitigs-pop-bubbles: rounds of unitigs, links, each enabled rule on that same graph and one mask of
// the k-mers of the tips and the popped arms through the host forms, before anything is written.  The mask stays set, so
// what write_unitigs and write_unitigs_map compute afterwards is the simplified graph.  Without --unitigs-pop-bubbles
// this is the tip loop as it always was, four-field report included; --unitigs-pop-bulges adds the bulge rule on that same
// graph, its pops to the same mask and a field to the report; --unitigs-drop-weak adds the weak rule the same way, with two
// fields at the end of the report's lines.
int simplify_unitigs(const Options &o, cfrk_ctx *ctx) {
  std::string report, bubbles, bulges, weaks;
  const uint32_t rounds = (o.pop_bubbles || o.pop_bulges || o.drop_weak) ? o.simplify_rounds : o.tip_rounds;
  UnitigGraph next;                                       // --simplify-recompact: the next round's unitigs, when the last one made them
  bool have_next = false;
  for (uint32_t round = 1; round <= rounds; ++round) {
    int64_t n_tips = 0, n_pop = 0, n_bulges = 0, n_weak = 0;
    cfrk_weak_stats weak_stats = {0, 0, 0};
    UnitigGraph g;
    int rc;
    if (have_next) {
      g = std::move(next);
      next = UnitigGraph();
      have_next = false;
      if ((rc = g.fetch_links(ctx, o.unitigs_min_count))) return rc;
    } else if ((rc = g.fetch(ctx, o.unitigs_min_count, true))) return rc;
    const int64_t nS = g.nS;
    std::vector<uint8_t> tip((size_t)nS);
    if (o.clip_tips &&
        (rc = cfrk_global_unitig_tips(ctx, g.rec.data(), nS, g.link_ptr.data(), g.links.data(), g.n_links, o.tip_max_kmers ? o.tip_max_kmers : (uint32_t)o.k,
                                      o.tip_ratio_q8, tip.data(), &n_tips))) return die(ctx, rc, "cfrk_global_unitig_tips");
    if (o.pop_bubbles) {
      std::vector<uint8_t> pop((size_t)nS);
      std::vector<uint32_t> partner((size_t)nS);
      if ((rc = cfrk_global_unitig_bubbles(ctx, g.rec.data(), nS, g.link_ptr.data(), g.links.data(), g.n_links,
                                           o.bubble_max_kmers ? o.bubble_max_kmers : (uint32_t)o.k, o.bubble_max_diff, o.bubble_ratio_q8,
                                           pop.data(), partner.data(), &n_pop))) return die(ctx, rc, "cfrk_global_unitig_bubbles");
      if (o.bubble_report && n_pop)
        format_into(bubbles, [&](char *out, size_t room) {
          return cfrk_host_format_bubbles(round, g.data.data(), g.start.data(), g.length.data(), g.rec.data(), nS, pop.data(), partner.data(), out, room);
        });
      for (size_t j = 0; j < (size_t)nS; ++j) tip[j] |= pop[j];       // (a popped unitig is never a tip: the rules' sets are disjoint)
    }
    if (o.pop_bulges) {
      std::vector<uint8_t> pop((size_t)nS);
      std::vector<int64_t> path_ptr((size_t)nS + 1);
      std::vector<uint32_t> path;
      int64_t n_path = 0;
      cfrk_bulge_stats stats;
      const uint32_t max_kmers = o.bulge_max_kmers ? o.bulge_max_kmers : (uint32_t)o.k;
      const uint64_t reach = (uint64_t)max_kmers + o.bulge_max_diff;
      const uint32_t max_hops = o.bulge_max_hops ? o.bulge_max_hops : (uint32_t)(reach < CFRK_BULGE_MAX_HOPS ? reach : CFRK_BULGE_MAX_HOPS);
      rc = sized_call([&] { return cfrk_global_unitig_bulges(ctx, g.rec.data(), nS, g.link_ptr.data(), g.links.data(), g.n_links, max_kmers, o.bulge_max_diff,
                                                             max_hops, o.bulge_max_visits, o.bulge_ratio_q8, pop.data(), nullptr, path_ptr.data(),
                                                             path.data(), path.size(), &n_path, &stats); },
                      [&] { path.resize((size_t)n_path); });
      if (rc) return die(ctx, rc, "cfrk_global_unitig_bulges");
      n_bulges = stats.popped;
      if (o.bulge_report && n_bulges)
        format_into(bulges, [&](char *out, size_t room) {
          return cfrk_host_format_bulges(round, g.data.data(), g.start.data(), g.length.data(), g.rec.data(), nS, pop.data(), path_ptr.data(), path.data(),
                                         o.k, out, room);
        });
      for (size_t j = 0; j < (size_t)nS; ++j) tip[j] |= pop[j];       // (disjoint from the tips; a bubble's arm may be popped by both rules)
    }
    if (o.drop_weak) {
      std::vector<uint8_t> weak((size_t)nS);
      if ((rc = cfrk_global_unitig_weak(ctx, g.rec.data(), nS, g.link_ptr.data(), g.links.data(), g.n_links, o.weak_max_kmers ? o.weak_max_kmers : (uint32_t)o.k,
                                        o.weak_ratio_q8, o.weak_iso_max_set ? o.weak_iso_max_kmers : 2u * (uint32_t)o.k, o.weak_iso_mean_q8, weak.data(),
                                        &weak_stats))) return die(ctx, rc, "cfrk_global_unitig_weak");
      n_weak = weak_stats.connections + weak_stats.isolated;
      if (o.weak_report && n_weak)
        format_into(weaks, [&](char *out, size_t room) {
          return cfrk_host_format_weak(round, g.data.data(), g.start.data(), g.length.data(), g.rec.data(), nS, weak.data(), out, room);
        });
      for (size_t j = 0; j < (size_t)nS; ++j) tip[j] |= weak[j] ? 1 : 0;    // (disjoint from the tips; a bubble's arm may be a connection too)
    }
    if ((n_tips || n_pop || n_bulges || n_weak) && (rc = cfrk_global_mask_unitigs(ctx, g.data.data(), g.start.data(), g.length.data(), g.nN, nS, tip.data())))
      return die(ctx, rc, "cfrk_global_mask_unitigs");
    uint64_t masked = 0;
    if ((rc = cfrk_global_mask_count(ctx, &masked))) return die(ctx, rc, "cfrk_global_mask_count");
    char line[192];
    int at;
    if (o.pop_bulges)
      at = snprintf(line, sizeof line, "%u\t%lld\t%lld\t%lld\t%lld\t%llu\n", round, (long long)nS, (long long)n_tips, (long long)n_pop, (long long)n_bulges,
               (unsigned long long)masked);
    else if (o.pop_bubbles)
      at = snprintf(line, sizeof line, "%u\t%lld\t%lld\t%lld\t%llu\n", round, (long long)nS, (long long)n_tips, (long long)n_pop, (unsigned long long)masked);
    else
      at = snprintf(line, sizeof line, "%u\t%lld\t%lld\t%llu\n", round, (long long)nS, (long long)n_tips, (unsigned long long)masked);
    if (o.drop_weak)                                      // (over the line's '\n': two fields more)
      snprintf(line + at - 1, sizeof line - (size_t)(at - 1), "\t%lld\t%lld\n", (long long)weak_stats.connections, (long long)weak_stats.isolated);
    report += line;
    if (!n_tips && !n_pop && !n_bulges && !n_weak) break;
    if (o.simplify_recompact && round < rounds) {
      if ((rc = g.compact_into(ctx, tip.data(), &next))) return rc;
      have_next = true;
    }
  }
  if (o.weak_report) { if (const int rc = write_file(o.weak_report, weaks)) return rc; }
  if (o.bulge_report) { if (const int rc = write_file(o.bulge_report, bulges)) return rc; }
  if (o.bubble_report) { if (const int rc = write_file(o.bubble_report, bubbles)) return rc; }
  return o.tip_report ? write_file(o.tip_report, report) : 0;
}

namespace {

// the components of a graph that has its links, through the host form: a sizes-only call, then a table of that size
int fetch_components(cfrk_ctx *ctx, const UnitigGraph &g, std::vector<uint32_t> *comp, std::vector<cfrk_unitig_component> *table) {
  comp->resize((size_t)g.nS);
  int64_t n = 0;
  cfrk_component_stats stats;
  const int rc = sized_call([&] { return cfrk_global_unitig_components(ctx, g.rec.data(), g.nS, g.link_ptr.data(), g.links.data(), g.n_links, nullptr,
                                                                        comp->data(), table->data(), table->size(), &n, &stats); },
                            [&] { table->resize((size_t)n); });
  return rc ? die(ctx, rc, "cfrk_global_unitig_components") : 0;
}

// --unitigs-component-tags: the CC:i: tags into a text that is already formatted (cfrk_host_tag_components)
void tag_components(std::string &buf, bool gfa, const std::vector<uint32_t> &comp) {
  std::string tagged;
  format_into(tagged, [&](char *out, size_t room) {
    return cfrk_host_tag_components(buf.data(), buf.size(), gfa ? 1 : 0, comp.data(), (int64_t)comp.size(), out, room);
  });
  buf.swap(tagged);
}

}  // namespace

// --unitigs-min-component-kmers N: unitigs, links and components of the graph as it stands (after any loop), then one mask
// of every unitig of a component of fewer than N k-mers.  The mask stays set: what is written afterwards is what is left.
int drop_small_components(const Options &o, cfrk_ctx *ctx) {
  UnitigGraph g;
  int rc;
  if ((rc = g.fetch(ctx, o.unitigs_min_count, true))) return rc;
  std::vector<uint32_t> comp;
  std::vector<cfrk_unitig_component> table;
  if ((rc = fetch_components(ctx, g, &comp, &table))) return rc;
  std::vector<uint8_t> drop((size_t)g.nS);
  bool any = false;
  for (size_t j = 0; j < (size_t)g.nS; ++j) any |= (drop[j] = table[comp[j]].n_kmers < o.min_component_kmers ? 1 : 0) != 0;
  if (any && (rc = cfrk_global_mask_unitigs(ctx, g.data.data(), g.start.data(), g.length.data(), g.nN, g.nS, drop.data())))
    return die(ctx, rc, "cfrk_global_mask_unitigs");
  return 0;
}

int write_unitigs(const Options &o, cfrk_ctx *ctx) {
  if (!o.unitigs_out && o.link_support) return 0;         // (GFILE alone, with the RC tags: write_unitigs_map fetches the graph and writes it)
  UnitigGraph g;
  const bool with_links = o.unitigs_links || o.unitigs_gfa || o.unitigs_components || o.component_tags;
  int rc;
  if ((rc = g.fetch(ctx, o.unitigs_min_count, with_links))) return rc;
  std::vector<uint32_t> comp;
  if (o.unitigs_components || o.component_tags) {
    std::vector<cfrk_unitig_component> table;
    if ((rc = fetch_components(ctx, g, &comp, &table))) return rc;
    if (o.unitigs_components) {
      std::string buf;
      format_into(buf, [&](char *out, size_t room) { return cfrk_host_format_components(table.data(), (int64_t)table.size(), o.k, out, room); });
      if ((rc = write_file(o.unitigs_components, buf))) return rc;
    }
  }
  if (o.unitigs_out) {
    const int64_t *lp = o.unitigs_links ? g.link_ptr.data() : nullptr;     // (without --unitigs-links: the bytes as they were)
    std::string buf;
    format_into(buf, [&](char *out, size_t room) {
      return with_links ? cfrk_host_format_unitigs_links(g.data.data(), g.start.data(), g.length.data(), g.rec.data(), g.nS, lp, g.links.data(), out, room)
                        : cfrk_host_format_unitigs(g.data.data(), g.start.data(), g.length.data(), g.rec.data(), g.nS, out, room);
    });
    if (o.component_tags) tag_components(buf, false, comp);
    if ((rc = write_file(o.unitigs_out, buf))) return rc;
  }
  if (o.unitigs_gfa && !o.link_support) {                 // (--unitigs-link-support: write_unitigs_map writes GFILE, with the RC tags)
    std::string buf;
    format_into(buf, [&](char *out, size_t room) {
      return cfrk_host_format_gfa(g.data.data(), g.start.data(), g.length.data(), g.rec.data(), g.nS, g.link_ptr.data(), g.links.data(), o.k, out, room);
    });
    if (o.component_tags) tag_components(buf, true, comp);
    if ((rc = write_file(o.unitigs_gfa, buf))) return rc;
  }
  return 0;
}

// --unitigs-map QFILE --unitigs-map-out MFILE: the unitigs into device arrays (a sizes-only call, then arrays of that
// size), where they stay; the position map from them (cfrk_global_unitig_index_device); the hits of QFILE's reads q
// (cfrk_global_read_hits) as GAF, the segment names those of --unitigs-gfa (cfrk_host_format_gaf).
// --unitigs-map-paths, --unitigs-link-support, --unitigs-map-stats: the hits joined across the links of that same graph
// (cfrk_global_read_paths); MFILE then holds one line per path (cfrk_host_format_gaf_paths), GFILE the RC:i: tags
// (cfrk_host_format_gfa_support), SFILE "reads hits paths steps gaps unlinked"
int write_unitigs_map(const Options &o, cfrk_ctx *ctx, const cfrk_batch &q) {
  int64_t nN = 0, nS = 0;
  int rc = cfrk_global_unitigs_device(ctx, o.unitigs_min_count, nullptr, 0, nullptr, nullptr, nullptr, 0, &nN, &nS);
  if (rc && rc != CFRK_ERR_SMALL_BUF) return die(ctx, rc, "cfrk_global_unitigs_device");
  void *d[4] = {nullptr, nullptr, nullptr, nullptr};      // data, start, length, records
  DeviceBufs bufs(ctx);
  std::vector<int32_t> ulen((size_t)nS);
  if (nS > 0) {
    const size_t bytes[4] = {(size_t)nN, (size_t)nS * 8, (size_t)nS * 4, (size_t)nS * sizeof(cfrk_unitig)};
    for (int j = 0; j < 4; ++j)
      if ((rc = bufs.alloc(bytes[j], &d[j]))) return die(ctx, rc, "cfrk_device_alloc");
    if ((rc = cfrk_global_unitigs_device(ctx, o.unitigs_min_count, (int8_t *)d[0], (uint64_t)nN, (int64_t *)d[1], (int32_t *)d[2],
                                         (cfrk_unitig *)d[3], (uint64_t)nS, &nN, &nS))) return die(ctx, rc, "cfrk_global_unitigs_device");
  }
  if ((rc = cfrk_global_unitig_index_device(ctx, o.unitigs_min_count, (const int8_t *)d[0], (const int64_t *)d[1], (const int32_t *)d[2],
                                            nN, nS))) return die(ctx, rc, "cfrk_global_unitig_index_device");
  if (nS > 0 && (rc = cfrk_memcpy_d2h(ctx, ulen.data(), d[2], (size_t)nS * 4))) return die(ctx, rc, "cfrk_memcpy_d2h");
  std::vector<int64_t> hit_ptr((size_t)q.nS + 1);
  std::vector<cfrk_read_hit> hits;
  int64_t n_hits = 0;
  rc = sized_call([&] { return cfrk_global_read_hits(ctx, q.data, q.start, q.length, q.nN, q.nS, hit_ptr.data(), hits.data(), hits.size(), &n_hits); },
                  [&] { hits.resize((size_t)n_hits); });
  if (rc) return die(ctx, rc, "cfrk_global_read_hits");
  std::string buf;
  if (o.map_components) {                                 // RFILE: the reads by component, on the graph that is written
    UnitigGraph cg;
    if ((rc = cg.fetch(ctx, o.unitigs_min_count, true))) return rc;
    std::vector<uint32_t> comp;
    std::vector<cfrk_unitig_component> table;
    if ((rc = fetch_components(ctx, cg, &comp, &table))) return rc;
    std::vector<cfrk_read_component> rows((size_t)q.nS);
    cfrk_read_component_stats rstats;
    if ((rc = cfrk_global_read_components(ctx, hit_ptr.data(), q.nS, hits.data(), n_hits, comp.data(), cg.nS, rows.data(), &rstats)))
      return die(ctx, rc, "cfrk_global_read_components");
    for (const cfrk_read_component &r : rows) {
      char line[64];
      if (r.comp == CFRK_COMP_NONE) snprintf(line, sizeof line, "*\t*\t0\t%u\n", r.flags);
      else snprintf(line, sizeof line, "%u\t%u\t%u\t%u\n", r.comp, r.hit, r.n_windows, r.flags);
      buf += line;
    }
    if ((rc = write_file(o.map_components, buf))) return rc;
    buf.clear();
  }
  if (!o.map_paths && !o.link_support && !o.map_stats) {
    format_into(buf, [&](char *out, size_t room) { return cfrk_host_format_gaf(q.length, q.nS, hit_ptr.data(), hits.data(), ulen.data(), o.k, out, room); });
    return write_file(o.unitigs_map_out, buf);
  }
  UnitigGraph g;
  if ((rc = g.fetch(ctx, o.unitigs_min_count, true))) return rc;
  std::vector<int64_t> path_ptr((size_t)q.nS + 1);
  std::vector<cfrk_read_path> paths;
  std::vector<uint32_t> support(o.link_support ? (size_t)g.n_links : 0);
  int64_t n_paths = 0;
  cfrk_path_stats stats;
  // a sizes-only call without support, then the call that fits: the steps are counted once
  auto call = [&](uint32_t *sup) {
    return cfrk_global_read_paths(ctx, hit_ptr.data(), q.nS, hits.data(), n_hits, g.rec.data(), g.nS, g.link_ptr.data(), g.links.data(), g.n_links,
                                  path_ptr.data(), paths.data(), paths.size(), &n_paths, sup, &stats);
  };
  rc = call(nullptr);
  if (!rc || rc == CFRK_ERR_SMALL_BUF) {
    paths.resize((size_t)n_paths);
    rc = call(o.link_support ? support.data() : nullptr);
  }
  if (rc) return die(ctx, rc, "cfrk_global_read_paths");
  format_into(buf, [&](char *out, size_t room) {
    return o.map_paths ? cfrk_host_format_gaf_paths(q.length, q.nS, hit_ptr.data(), hits.data(), path_ptr.data(), paths.data(), ulen.data(), o.k, out, room)
                       : cfrk_host_format_gaf(q.length, q.nS, hit_ptr.data(), hits.data(), ulen.data(), o.k, out, room);
  });
  if ((rc = write_file(o.unitigs_map_out, buf))) return rc;
  if (o.link_support) {
    buf.clear();
    format_into(buf, [&](char *out, size_t room) {
      return cfrk_host_format_gfa_support(g.data.data(), g.start.data(), g.length.data(), g.rec.data(), g.nS, g.link_ptr.data(), g.links.data(),
                                          support.data(), o.canonical ? 1 : 0, o.k, out, room);
    });
    if (o.component_tags) {                               // (GFILE is written here: the CC tags as write_unitigs puts them)
      std::vector<uint32_t> comp;
      std::vector<cfrk_unitig_component> table;
      if ((rc = fetch_components(ctx, g, &comp, &table))) return rc;
      tag_components(buf, true, comp);
    }
    if ((rc = write_file(o.unitigs_gfa, buf))) return rc;
  }
  if (o.map_stats) {
    char line[160];
    snprintf(line, sizeof line, "%lld\t%lld\t%llu\t%llu\t%llu\t%llu\n", (long long)q.nS, (long long)n_hits, (unsigned long long)stats.n_paths,
             (unsigned long long)stats.n_steps, (unsigned long long)stats.n_gaps, (unsigned long long)stats.n_unlinked);
    if ((rc = write_file(o.map_stats, line))) return rc;
  }
  return 0;
}
