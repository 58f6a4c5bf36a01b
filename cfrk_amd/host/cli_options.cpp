// cli_options.cpp -- the options of the `cfrk` command: one table row per option, one interpreter per kind of value, and
// the rules between options.  Needs cfrk_abi.h for its constants alone: this unit and cfrk_host.cpp link without
// libcfrk_hip.so (tools/cli_options_host_check.cpp runs them under the sanitizers).
#include "cli_options.h"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <string>
#include <thread>

#include "cfrk_host.h"

namespace {

// a count option's value: decimal digits only, below 2^32
bool parse_count(const char *v, uint32_t *out) {
  if (!*v || strlen(v) > 10) return false;
  uint64_t x = 0;
  for (const char *p = v; *p; ++p) {
    if (*p < '0' || *p > '9') return false;
    x = x * 10 + (uint64_t)(*p - '0');
  }
  if (x > 0xFFFFFFFFull) return false;
  *out = (uint32_t)x;
  return true;
}

// FLAG takes no value.  INT is read as the reference reads its numbers (atoi, unchecked); COUNT0 / COUNT1 are counts from 0 / 1
// to 2^32 - 1; RATIO is a number from 0 to 256 kept in 256ths; RANGED an integer from lo to hi; WORD one of up to three words
enum Kind { FLAG, STR, INT, COUNT0, COUNT1, RATIO, RANGED, WORD };
struct Word { const char *word; int value; };
typedef bool Options::*Set;
typedef void (*Hook)(Options &);
struct Row {
  const char *name;
  Kind kind;
  union { bool Options::*b; const char *Options::*s; int Options::*i; uint32_t Options::*u; long long Options::*l; };
  Set set;                  // raised when the option is given (NULL: none)
  Hook hook;                // what else the option implies, run after the value is stored (NULL: nothing)
  long long lo, hi;         // RANGED
  const char *noun;         // RANGED: what the refusal says is needed
  Word words[3];            // WORD
};
Row row(const char *name, Kind kind, Set set, Hook hook) { Row r{}; r.name = name; r.kind = kind; r.set = set; r.hook = hook; return r; }
Row flag(const char *name, bool Options::*m, Set set = nullptr, Hook hook = nullptr) { Row r = row(name, FLAG, set, hook); r.b = m; return r; }
Row str(const char *name, const char *Options::*m, Set set = nullptr) { Row r = row(name, STR, set, nullptr); r.s = m; return r; }
Row integer(const char *name, int Options::*m, Hook hook = nullptr) { Row r = row(name, INT, nullptr, hook); r.i = m; return r; }
Row count(const char *name, uint32_t least, uint32_t Options::*m, Set set = nullptr, Hook hook = nullptr) { Row r = row(name, least ? COUNT1 : COUNT0, set, hook); r.u = m; return r; }
Row ratio(const char *name, uint32_t Options::*m, Set set) { Row r = row(name, RATIO, set, nullptr); r.u = m; return r; }
Row ranged(const char *name, long long lo, long long hi, const char *noun, long long Options::*m, Set set) {
  Row r = row(name, RANGED, set, nullptr); r.l = m; r.lo = lo; r.hi = hi; r.noun = noun; return r;
}
Row word(const char *name, int Options::*m, std::initializer_list<Word> words, Set set = nullptr, Hook hook = nullptr) {
  Row r = row(name, WORD, set, hook); r.i = m;
  size_t n = 0;
  for (const Word &w : words) r.words[n++] = w;
  return r;
}

#define TEXT_OF_(x) #x
#define TEXT_OF(x) TEXT_OF_(x)
typedef Options O;
const Row TABLE[] = {
  flag("--all-chunks", &O::all_chunks), flag("--native", &O::native), flag("--global", &O::global), flag("--canonical", &O::canonical),
  flag("--sparse", &O::sparse), flag("--binary", &O::binary), flag("--timing", &O::timing),
  integer("--parse-threads", &O::parse_threads, [](O &o) { cfrk_host_set_parse_threads(o.parse_threads); }),
  flag("--same-device", &O::same_device),   // rehearsal: every "device" is --device
  integer("--device", &O::device), integer("--gpus", &O::gpus), integer("--batch", &O::batch_n),
  flag("--histo-only", &O::histo_only), flag("--estimate", &O::estimate), flag("--estimate-only", &O::estimate_only),
  flag("--auto-hint", &O::auto_hint), flag("--device-parse", &O::device_parse),
  word("--text-copy", &O::text_copy_plain, {{"plain", 1}, {"staged", 0}}),
  word("--format", &O::format, {{"fasta", CFRK_FORMAT_FASTA}, {"fastq", CFRK_FORMAT_FASTQ}, {"auto", -1}}),
  ranged("--min-qual", 0, CFRK_FASTQ_MAX_QUAL, "an integer from 0 to " TEXT_OF(CFRK_FASTQ_MAX_QUAL), &O::min_qual, &O::min_qual_set),
  flag("--query-only", &O::query_only), flag("--paired", &O::paired),
  word("--pair-check", &O::pair_check, {{"on", 1}, {"off", 0}}, &O::pair_opt_set),
  word("--pair-mode", &O::pair_mode, {{"either", CFRK_PAIR_EITHER}, {"both", CFRK_PAIR_BOTH}}, &O::pair_mode_set),
  str("--query2", &O::query2), str("--query", &O::query), str("--query-out", &O::query_out), str("--query-db", &O::query_db),
  str("--query-stats", &O::query_stats), count("--stats-below", 0, &O::stats_below, &O::stats_below_set),
  str("--filter-out", &O::filter_out), str("--filter-out2", &O::filter_out2), str("--filter-orphans", &O::filter_orphans),
  flag("--filter-names", &O::filter_names, &O::filter_opt_set),
  word("--filter-format", &O::filter_format, {{"fasta", CFRK_TEXT_FASTA}, {"fastq", CFRK_TEXT_FASTQ}}, &O::filter_opt_set,
       [](O &o) { if (o.filter_format == CFRK_TEXT_FASTQ) o.filter_names = true; }),
  word("--filter-trim", &O::filter_trim, {{"longest", CFRK_SPAN_LONGEST}, {"prefix", CFRK_SPAN_PREFIX}, {"none", -1}}, &O::filter_opt_set),
  ranged("--filter-min-len", 0, 0x7FFFFFFFll, "a length (an integer from 0 to 2147483647)", &O::filter_min_len, &O::filter_opt_set),
  count("--filter-min-count", 0, &O::filter_min_count, &O::filter_opt_set), count("--filter-max-count", 0, &O::filter_max_count, &O::filter_opt_set),
  count("--filter-min-median", 0, &O::filter_min_median, &O::filter_opt_set, [](O &o) { o.filter_median = true; }),
  count("--filter-max-median", 0, &O::filter_max_median, &O::filter_opt_set, [](O &o) { o.filter_median = true; }),
  str("--correct-out", &O::correct_out), str("--correct-out2", &O::correct_out2),
  flag("--correct-names", &O::correct_names, &O::correct_opt_set),
  word("--correct-format", &O::correct_format, {{"fasta", CFRK_TEXT_FASTA}, {"fastq", CFRK_TEXT_FASTQ}}, &O::correct_opt_set,
       [](O &o) { if (o.correct_format == CFRK_TEXT_FASTQ) o.correct_names = true; }),
  str("--correct-report", &O::correct_report, &O::correct_opt_set),
  count("--correct-min-count", 0, &O::correct_min_count, &O::correct_opt_set, [](O &o) { o.correct_min_count_set = true; }),
  str("--normalize-out", &O::normalize_out), flag("--normalize-names", &O::normalize_names, &O::normalize_opt_set),
  word("--normalize-format", &O::normalize_format, {{"fasta", CFRK_TEXT_FASTA}, {"fastq", CFRK_TEXT_FASTQ}}, &O::normalize_opt_set,
       [](O &o) { o.normalize_names = true; }),
  ranged("--normalize-batch", 1, LLONG_MAX, "a number of reads (an integer from 1)", &O::normalize_batch, &O::normalize_opt_set),
  count("--normalize-cutoff", 0, &O::normalize_cutoff, &O::normalize_opt_set, [](O &o) { o.normalize_cutoff_set = true; }),
  str("--histo", &O::histo),
  count("--min-count", 0, &O::min_count, &O::range_set),     // (0 reads as 1: cfrk_global_export_range)
  count("--max-count", 0, &O::max_count, &O::range_set),
  flag("--unitigs-links", &O::unitigs_links), flag("--unitigs-clip-tips", &O::clip_tips),
  str("--tip-report", &O::tip_report), ratio("--tip-ratio", &O::tip_ratio_q8, &O::tip_opt_set),
  count("--tip-max-kmers", 1, &O::tip_max_kmers, &O::tip_opt_set),
  count("--tip-rounds", 1, &O::tip_rounds, &O::tip_opt_set, [](O &o) { o.tip_rounds_set = true; }),
  flag("--unitigs-pop-bubbles", &O::pop_bubbles),
  str("--bubble-report", &O::bubble_report, &O::bubble_opt_set), ratio("--bubble-ratio", &O::bubble_ratio_q8, &O::bubble_opt_set),
  count("--bubble-max-kmers", 1, &O::bubble_max_kmers, &O::bubble_opt_set), count("--bubble-max-diff", 0, &O::bubble_max_diff, &O::bubble_opt_set),
  count("--simplify-rounds", 1, &O::simplify_rounds, &O::simplify_rounds_set),
  flag("--unitigs-pop-bulges", &O::pop_bulges), flag("--simplify-recompact", &O::simplify_recompact),
  str("--bulge-report", &O::bulge_report, &O::bulge_opt_set), ratio("--bulge-ratio", &O::bulge_ratio_q8, &O::bulge_opt_set),
  count("--bulge-max-kmers", 1, &O::bulge_max_kmers, &O::bulge_opt_set), count("--bulge-max-diff", 0, &O::bulge_max_diff, &O::bulge_opt_set),
  count("--bulge-max-hops", 1, &O::bulge_max_hops, &O::bulge_opt_set), count("--bulge-max-visits", 0, &O::bulge_max_visits, &O::bulge_opt_set),
  flag("--unitigs-drop-weak", &O::drop_weak),
  str("--weak-report", &O::weak_report, &O::weak_opt_set), ratio("--weak-ratio", &O::weak_ratio_q8, &O::weak_opt_set),
  count("--weak-max-kmers", 1, &O::weak_max_kmers, &O::weak_opt_set),
  count("--weak-iso-max-kmers", 0, &O::weak_iso_max_kmers, &O::weak_opt_set, [](O &o) { o.weak_iso_max_set = true; }),
  ratio("--weak-iso-mean", &O::weak_iso_mean_q8, &O::weak_opt_set),
  str("--unitigs-out", &O::unitigs_out), str("--unitigs-gfa", &O::unitigs_gfa), str("--unitigs-map", &O::unitigs_map),
  str("--unitigs-map-out", &O::unitigs_map_out), count("--unitigs-min-count", 0, &O::unitigs_min_count, &O::unitigs_opt_set),
  flag("--unitigs-map-paths", &O::map_paths), flag("--unitigs-link-support", &O::link_support), str("--unitigs-map-stats", &O::map_stats),
  str("--unitigs-components", &O::unitigs_components), flag("--unitigs-component-tags", &O::component_tags), str("--unitigs-map-components", &O::map_components),
  count("--unitigs-min-component-kmers", 0, &O::min_component_kmers, &O::component_opt_set),
};

// the value v of row r into o; 1 (the refusal printed) when it is not one the kind takes
int store(const Row &r, const char *v, Options &o) {
  switch (r.kind) {
  case FLAG: o.*r.b = true; return 0;
  case STR: o.*r.s = v; return 0;
  case INT: o.*r.i = atoi(v); return 0;
  case COUNT0:
  case COUNT1: {
    uint32_t x;
    const uint32_t least = r.kind == COUNT1 ? 1u : 0u;
    if (!parse_count(v, &x) || x < least) { fprintf(stderr, "cfrk: %s needs a count (an integer from %u to 4294967295), not '%s'\n", r.name, least, v); return 1; }
    o.*r.u = x;
    return 0;
  }
  case RATIO: {
    char *end = nullptr;
    const double x = strtod(v, &end);
    if (end == v || *end || !(x >= 0.0 && x <= 256.0)) { fprintf(stderr, "cfrk: %s needs a number from 0 to 256, not '%s'\n", r.name, v); return 1; }
    o.*r.u = (uint32_t)(x * 256.0 + 0.5);
    return 0;
  }
  case RANGED: {
    char *end = nullptr;
    const long long x = strtoll(v, &end, 10);
    if (!*v || *end || x < r.lo || x > r.hi) { fprintf(stderr, "cfrk: %s needs %s, not '%s'\n", r.name, r.noun, v); return 1; }
    o.*r.l = x;
    return 0;
  }
  case WORD: {
    std::string list;                                    // "a or b", "a, b or c"
    for (size_t j = 0; j < 3 && r.words[j].word; ++j) {
      if (!strcmp(v, r.words[j].word)) { o.*r.i = r.words[j].value; return 0; }
      if (j) list += (j + 1 < 3 && r.words[j + 1].word) ? ", " : " or ";
      list += r.words[j].word;
    }
    fprintf(stderr, "cfrk: %s takes %s, not '%s'\n", r.name, list.c_str(), v);
    return 1;
  }
  }
  return 0;
}

int refuse(const char *msg) {
  fprintf(stderr, "cfrk: %s\n", msg);
  return 1;
}

}  // namespace

const char *option_at(size_t i, bool *takes_value) {
  if (i >= sizeof TABLE / sizeof TABLE[0]) return nullptr;
  *takes_value = TABLE[i].kind != FLAG;
  return TABLE[i].name;
}

int parse_options(int argc, char **argv, Options &o) {
  for (int i = 1; i < argc; ++i) {
    const Row *r = nullptr;
    for (const Row &t : TABLE) if (!strcmp(argv[i], t.name)) { r = &t; break; }
    if (!r) {
      // (these three families are closed: a misspelt member is not a file name)
      if (!strncmp(argv[i], "--filter-", 9) || !strncmp(argv[i], "--correct-", 10) || !strncmp(argv[i], "--normalize-", 12)) {
        fprintf(stderr, "cfrk: unknown option %s\n", argv[i]);
        return 1;
      }
      o.pos.push_back(argv[i]);
      continue;
    }
    if (r->kind != FLAG && i + 1 >= argc) { fprintf(stderr, "cfrk: %s needs a value\n", argv[i]); return 1; }
    if (store(*r, r->kind == FLAG ? nullptr : argv[++i], o)) return 1;
    if (r->set) o.*r->set = true;
    if (r->hook) r->hook(o);
  }
  return 0;
}

// (refused here: before the input is parsed or a device is opened)
int check_options(const Options &o) {
  const bool batch = o.batch_n >= 0;
  const bool not_global_on_one = !o.global || o.gpus > 1 || batch || o.sparse;           // what the graph outputs cannot run with
  const bool graph_out = o.unitigs_out || o.unitigs_gfa || o.unitigs_map;
  auto needs_global_on_one = [](const char *name) {
    fprintf(stderr, "cfrk: %s needs --global on one device: not with --gpus above 1, --batch or --sparse\n", name);
    return 1;
  };
  if (o.unitigs_out && not_global_on_one) return needs_global_on_one("--unitigs-out");
  if (o.unitigs_gfa && not_global_on_one) return needs_global_on_one("--unitigs-gfa");
  if ((o.unitigs_map != nullptr) != (o.unitigs_map_out != nullptr)) return refuse("--unitigs-map QFILE and --unitigs-map-out MFILE go together");
  if (o.unitigs_map && not_global_on_one) return needs_global_on_one("--unitigs-map");
  if (o.map_paths && !o.unitigs_map) return refuse("--unitigs-map-paths needs --unitigs-map QFILE");
  if (o.link_support && !(o.unitigs_map && o.unitigs_gfa)) return refuse("--unitigs-link-support needs --unitigs-map QFILE and --unitigs-gfa GFILE");
  if (o.map_stats && !o.unitigs_map) return refuse("--unitigs-map-stats needs --unitigs-map QFILE");
  if (o.clip_tips && !graph_out) return refuse("--unitigs-clip-tips needs --unitigs-out UFILE, --unitigs-gfa GFILE or --unitigs-map QFILE");
  if (o.pop_bubbles && !graph_out) return refuse("--unitigs-pop-bubbles needs --unitigs-out UFILE, --unitigs-gfa GFILE or --unitigs-map QFILE");
  if (o.pop_bulges && !graph_out) return refuse("--unitigs-pop-bulges needs --unitigs-out UFILE, --unitigs-gfa GFILE or --unitigs-map QFILE");
  if (o.drop_weak && !graph_out) return refuse("--unitigs-drop-weak needs --unitigs-out UFILE, --unitigs-gfa GFILE or --unitigs-map QFILE");
  if (o.weak_opt_set && !o.drop_weak)
    return refuse("--weak-max-kmers, --weak-ratio, --weak-iso-max-kmers, --weak-iso-mean and --weak-report need --unitigs-drop-weak");
  if (o.bulge_opt_set && !o.pop_bulges)
    return refuse("--bulge-max-kmers, --bulge-max-diff, --bulge-max-hops, --bulge-max-visits, --bulge-ratio and --bulge-report need --unitigs-pop-bulges");
  if (o.simplify_recompact && !o.clip_tips && !o.pop_bubbles && !o.pop_bulges && !o.drop_weak)
    return refuse("--simplify-recompact needs --unitigs-clip-tips, --unitigs-pop-bubbles or --unitigs-pop-bulges");
  if (o.bulge_max_hops > CFRK_BULGE_MAX_HOPS) return refuse("--bulge-max-hops needs a count from 1 to " TEXT_OF(CFRK_BULGE_MAX_HOPS));
  if (o.bulge_max_visits > CFRK_BULGE_MAX_VISITS) return refuse("--bulge-max-visits needs a count from 0 to " TEXT_OF(CFRK_BULGE_MAX_VISITS));
  if ((o.bubble_opt_set && !o.pop_bubbles) || (o.simplify_rounds_set && !o.pop_bubbles && !o.pop_bulges && !o.drop_weak)) return refuse("--bubble-max-kmers, --bubble-max-diff, --bubble-ratio, --bubble-report and --simplify-rounds need --unitigs-pop-bubbles");
  if (o.tip_rounds_set && o.pop_bubbles) return refuse("--tip-rounds is the tip loop's own: with --unitigs-pop-bubbles the rounds are set by --simplify-rounds N");
  if (o.tip_rounds_set && o.pop_bulges) return refuse("--tip-rounds is the tip loop's own: with --unitigs-pop-bulges the rounds are set by --simplify-rounds N");
  if (o.tip_rounds_set && o.drop_weak) return refuse("--tip-rounds is the tip loop's own: with --unitigs-drop-weak the rounds are set by --simplify-rounds N");
  if ((o.tip_opt_set && !o.clip_tips) || (o.tip_report && !o.clip_tips && !o.pop_bubbles && !o.pop_bulges && !o.drop_weak)) return refuse("--tip-max-kmers, --tip-ratio, --tip-rounds and --tip-report need --unitigs-clip-tips");
  if (o.unitigs_links && !o.unitigs_out) return refuse("--unitigs-links needs --unitigs-out UFILE");
  if (o.unitigs_opt_set && !graph_out) return refuse("--unitigs-min-count needs --unitigs-out UFILE");
  if (o.unitigs_components && !o.unitigs_out) return refuse("--unitigs-components needs --unitigs-out UFILE");
  if (o.component_tags && !o.unitigs_out) return refuse("--unitigs-component-tags needs --unitigs-out UFILE");
  if (o.component_opt_set && !o.unitigs_out) return refuse("--unitigs-min-component-kmers needs --unitigs-out UFILE");
  if (o.map_components && !(o.unitigs_out && o.unitigs_map)) return refuse("--unitigs-map-components needs --unitigs-out UFILE and --unitigs-map QFILE");
  if (o.sparse && (o.global || o.binary || o.histo || o.histo_only || o.range_set || o.query || o.query_out || o.query_only || o.query_db ||
                   o.query_stats || o.stats_below_set || o.filter_out || o.filter_opt_set || o.correct_out || o.correct_opt_set))
    return refuse("--sparse is a per-read mode: not with --global, --binary, --histo, --query or --min-count / --max-count");
  if ((o.histo || o.histo_only || o.range_set) && !o.global) return refuse("--histo, --histo-only, --min-count and --max-count need --global");
  if ((o.estimate || o.estimate_only || o.auto_hint) && !o.global) return refuse("--estimate, --estimate-only and --auto-hint need --global");
  if (o.device_parse && (!o.global || o.gpus > 1 || batch)) return refuse("--device-parse needs --global on one device: not with --gpus above 1 or --batch");
  if (o.estimate_only && batch) return refuse("--estimate-only prints one estimate: not with --batch");
  if (o.histo_only && !o.histo) return refuse("--histo-only needs --histo FILE");
  if (o.min_count > o.max_count) {
    fprintf(stderr, "cfrk: --min-count %u is above --max-count %u\n", o.min_count, o.max_count);
    return 1;
  }
  if (o.histo && batch) return refuse("--histo writes one file: not with --batch");
  if (o.query && !o.global && !o.query_db) return refuse("--query needs --global or --query-db");
  if ((o.query_out || o.query_only || o.query_db) && !o.query) return refuse("--query-out, --query-only and --query-db need --query QFILE");
  if ((o.query_stats || o.stats_below_set) && !o.query) return refuse("--query-stats and --stats-below need --query QFILE");
  if (o.stats_below_set && !o.query_stats) return refuse("--stats-below needs --query-stats SFILE");
  if ((o.filter_out || o.filter_opt_set) && !o.query) return refuse("--filter-out and the --filter- options need --query QFILE");
  if (o.filter_opt_set && !o.filter_out) return refuse("the --filter- options need --filter-out FFILE");
  if (o.correct_opt_set && !o.correct_out) return refuse("the --correct- options need --correct-out CFILE");
  if (o.correct_out && !o.query) return refuse("--correct-out and the --correct- options need --query QFILE");
  if (o.correct_out && !o.correct_min_count_set) return refuse("--correct-out needs --correct-min-count T");
  // paired-end reads
  if (o.paired && o.query2) return refuse("--paired says the mates are interleaved in one file, --query2 that they are in two: one of them");
  if (o.query2 && o.normalize_out && !o.filter_out && !o.correct_out)
    return refuse("--normalize-out takes ONE input file: mates in two files are not supported, interleave them and say --paired");
  if (o.query2 && !o.query) return refuse("--query2 needs --query QFILE");
  if (o.paired && o.gpus > 1) return refuse("--paired runs on one device: not with --gpus above 1");
  if (o.paired && batch) return refuse("--paired reads one file: not with --batch");
  if (o.paired && !o.filter_out && !o.correct_out && !o.normalize_out) return refuse("--paired needs --filter-out FFILE, --correct-out CFILE or --normalize-out NFILE");
  if (o.query2 && !o.filter_out && !o.correct_out) return refuse("--query2 needs --filter-out FFILE or --correct-out CFILE");
  if (o.query2 && o.filter_out && !o.filter_out2) return refuse("--query2 needs --filter-out2 FFILE2 beside --filter-out");
  if (o.query2 && o.correct_out && !o.correct_out2) return refuse("--query2 needs --correct-out2 CFILE2 beside --correct-out");
  if ((o.filter_out2 && !(o.query2 && o.filter_out)) || (o.correct_out2 && !(o.query2 && o.correct_out)))
    return refuse("--filter-out2 and --correct-out2 receive QFILE2's reads: they need --query2 and --filter-out / --correct-out");
  if (o.filter_orphans && !(o.mates() && o.filter_out)) return refuse("--filter-orphans needs --paired or --query2, and --filter-out");
  if ((o.pair_opt_set && !o.mates()) || (o.pair_mode_set && !(o.paired && o.normalize_out)))
    return refuse("--pair-check needs --paired or --query2; --pair-mode needs --paired with --normalize-out");
  if (o.paired && o.normalize_out && (o.normalize_batch & 1)) {
    fprintf(stderr, "cfrk: --normalize-batch %lld: a round of --paired reads holds whole pairs, an even number\n", o.normalize_batch);
    return 1;
  }
  if (o.query && !o.query_out && !o.query_stats && !o.filter_out && !o.correct_out)
    return refuse("--query needs --query-out OFILE, --query-stats SFILE, --filter-out FFILE or --correct-out CFILE");
  if (o.correct_out && o.gpus > 1) return refuse("--correct-out runs on one device: not with --gpus above 1");
  if (o.filter_out && o.gpus > 1) return refuse("--filter-out runs on one device: not with --gpus above 1");
  if (o.query_stats && o.gpus > 1) return refuse("--query-stats runs on one device: not with --gpus above 1");
  if (o.query && batch) return refuse("--query writes one file: not with --batch");
  if (o.query_db && !o.pos.empty()) return refuse("--query-db takes no positional arguments");
  if (o.query_db && o.min_qual_set) return refuse("--min-qual applies to the FASTQ input that is counted: not with --query-db");
  if ((o.normalize_out || o.normalize_opt_set) && (!o.global || o.sparse)) return refuse("--normalize-out and the --normalize- options need --global");
  if (o.normalize_opt_set && !o.normalize_out) return refuse("the --normalize- options need --normalize-out NFILE");
  if (o.normalize_out && !o.normalize_cutoff_set) return refuse("--normalize-out needs --normalize-cutoff C");
  if (o.normalize_out && (o.gpus > 1 || batch || o.device_parse || o.query_db))
    return refuse("--normalize-out runs on one device and writes one file: not with --gpus above 1, --batch, --device-parse or --query-db");
  return 0;
}

int apply_positionals(Options &o) {
  if (o.pos.size() < 3) {
    // src/main.cu:239-243
    printf("Usage: ./cfrk [dataset.fasta] [file_out.cfrk] [k] <number of threads: Default 12> <chunkSize: Default 8192>");
    return 1;
  }
  o.k = atoi(o.pos[2]);
  if (o.sparse && (o.k < 1 || o.k > 32)) { fprintf(stderr, "cfrk: --sparse needs 1 <= k <= 32 (one-word keys), not %d\n", o.k); return 1; }
  if (o.sparse) { o.native = true; o.all_chunks = true; }   // clean parse, guarded semantics, every chunk
  if (o.pos.size() >= 4) o.threads = atoi(o.pos[3]);
  if (o.threads < 1) o.threads = 1;
  { const unsigned hw = std::thread::hardware_concurrency(); if (hw && (unsigned)o.threads > hw) o.threads = (int)hw; }
  if (o.pos.size() == 5) o.chunk_size = atol(o.pos[4]);     // argc == 6 in the reference
  if (o.chunk_size <= 0) return refuse("chunkSize must be positive");
  if (o.gpus < 1) return refuse("--gpus must be positive");
  if (o.batch_n == 0 || o.batch_n < -1) return refuse("--batch needs a positive file count");
  return 0;
}
