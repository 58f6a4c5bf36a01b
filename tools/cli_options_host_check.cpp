// cli_options_host_check.cpp -- the option parser and the cross-option rules of the `cfrk` command (cli_options.cpp)
// under the sanitizers, on the CPU, outside pytest.  Built and run as tools/bubbles_host_check.cpp is:
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       -o cli_options_host_check tools/cli_options_host_check.cpp cfrk_amd/host/cli_options.cpp cfrk_amd/host/cfrk_host.cpp
//   ./cli_options_host_check
//
// No libcfrk_hip.so: the option unit needs the ABI header for its constants alone.  Every argument is a heap block of
// exactly its length (so that a read past it is seen) and argv has exactly argc + 1 entries.  Fed: every option as the last
// argument (a value option there must be refused), every value option with awkward values -- the empty string, a lone
// "--", signs, 11-digit counts, values one past a bound -- values whose outcome is known, and a few hundred random vectors
// of options, values and positionals.  The refusals the parser prints go to stderr, as the command's do.  Prints one summary
// line; exit status 1 when an outcome is not the expected one.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../cfrk_amd/host/cli_options.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

static size_t vectors = 0, refused = 0, failures = 0;

// parse + rules + positionals on one argument vector: 0 when all three accept it, 1 when one refuses; o is what was parsed
static int run(const std::vector<std::string> &args, Options &o) {
  const int argc = (int)args.size() + 1;
  char **argv = (char **)malloc(((size_t)argc + 1) * sizeof(char *));
  for (int i = 0; i < argc; ++i) {
    const std::string &a = i ? args[(size_t)i - 1] : std::string("cfrk");
    argv[i] = (char *)malloc(a.size() + 1);
    memcpy(argv[i], a.c_str(), a.size() + 1);
  }
  argv[argc] = nullptr;
  int rc = parse_options(argc, argv, o);
  if (!rc) rc = check_options(o);
  if (!rc && !o.query_db) rc = apply_positionals(o);
  if (rc != 0 && rc != 1) { printf("status %d\n", rc); ++failures; }
  o.pos.clear();                       // (the positionals point into argv, which goes now; so do the paths: only numbers and flags are read afterwards)
  for (int i = 0; i < argc; ++i) free(argv[i]);
  free(argv);
  ++vectors;
  refused += (size_t)rc;
  return rc;
}

static void expect(bool ok, const char *what, const std::string &detail) {
  if (ok) return;
  printf("FAILED: %s (%s)\n", what, detail.c_str());
  ++failures;
}

int main() {
  std::vector<std::pair<std::string, bool>> table;
  bool takes = false;
  for (size_t i = 0; option_at(i, &takes); ++i) table.push_back({option_at(i, &takes), takes});
  expect(table.size() >= 70, "the table has its rows", std::to_string(table.size()));
  const std::vector<std::string> head = {"in.fasta", "out.cfrk", "15"};
  auto with = [&](std::vector<std::string> more) { std::vector<std::string> v = head; v.insert(v.end(), more.begin(), more.end()); return v; };

  // every option as the last argument, alone and behind --global
  for (const auto &t : table)
    for (int g = 0; g < 2; ++g) {
      Options o;
      const int rc = run(g ? with({"--global", t.first}) : with({t.first}), o);
      if (t.second) expect(rc == 1, "a value option without its value is refused", t.first);
    }
  // every value option with awkward values: whatever the answer, nothing is read out of bounds
  const char *awkward[] = {"", "--", "-", "+", "-1", "+1", "0", "1", "256", "256.0001", "257", "1e3", "nan", "inf", "4294967295", "4294967296",
                           "42949672950", "99999999999", "99999999999999999999", "9223372036854775808", " 1", "1 ", "0x10", "fastq", "FASTQ", "none"};
  for (const auto &t : table)
    if (t.second)
      for (const char *v : awkward) { Options o; run(with({"--global", t.first, v}), o); }
  // outcomes that are known
  {
    Options o;
    expect(run(with({"--global", "--unitigs-gfa", "g", "--unitigs-clip-tips", "--tip-ratio", "1.5", "--tip-max-kmers", "4294967295"}), o) == 0 &&
           o.tip_ratio_q8 == 384 && o.tip_max_kmers == 4294967295u && o.tip_opt_set && o.k == 15, "ratio in 256ths, the largest count", "tip");
  }
  for (const char *v : {"42949672950", "99999999999", "4294967296", "", "-0", "+5"}) {
    Options o;
    expect(run(with({"--global", "--min-count", v}), o) == 1, "a count out of range is refused", v);
  }
  {
    Options o;
    expect(run(with({"--global", "--", "", "--filter-"}), o) == 1, "an unknown --filter- option is refused", "--filter-");
  }
  {
    Options o;       // (a lone "--" and an empty string are positionals: five of them, the fifth is chunkSize, and 0 is refused)
    expect(run({"in", "out", "15", "--", ""}, o) == 1, "chunkSize from an empty fifth positional is refused", "--");
    Options p;
    expect(run({"in", "out", "15", "--"}, p) == 0 && p.k == 15 && p.threads == 1, "a lone -- is the threads positional", "--");
    Options q;
    expect(run({"--filter-format", "fastq", "--query", "q", "--filter-out", "f", "--global", "a", "b", "31"}, q) == 0 && q.filter_names &&
           q.filter_format == CFRK_TEXT_FASTQ && q.filter_opt_set && q.k == 31, "--filter-format fastq implies --filter-names", "hook");
    Options r;
    expect(run({"--query-db", "db", "--query", "q", "--query-out", "o"}, r) == 0, "--query-db takes no positionals", "db");
  }
  // random vectors: options with a value from the awkward or the plausible, flags, positionals
  const char *plausible[] = {"2", "20", "1.5", "fasta", "fastq", "on", "off", "both", "either", "plain", "longest", "auto", "file.txt"};
  for (int round = 0; round < 400; ++round) {
    std::vector<std::string> v;
    if (rnd() % 8) v = head;
    if (rnd() % 4) v.push_back("--global");
    for (uint64_t n = rnd() % 7; n > 0; --n) {
      const auto &t = table[(size_t)(rnd() % table.size())];
      if (rnd() % 16 == 0) { v.push_back(rnd() % 2 ? "" : "--"); continue; }
      v.push_back(t.first);
      if (t.second && rnd() % 12) v.push_back(rnd() % 4 ? plausible[rnd() % (sizeof plausible / sizeof *plausible)] : awkward[rnd() % (sizeof awkward / sizeof *awkward)]);
    }
    Options o;
    run(v, o);
  }
  if (failures) { printf("%zu failure(s)\n", failures); return 1; }
  printf("parser and rules held: %zu argument vectors over %zu options, %zu refused\n", vectors, table.size(), refused);
  return 0;
}
