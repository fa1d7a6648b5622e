// lookup_fsm_draft_check — host-only exercise of the drafter of constrained lookup decode (csrc/kh_lookup.h:
// kh_lookup_draft_fsm_core, over csrc/kh_fsm.h's host part): the named cases of tests/test_lookup_fsm.py, and random
// automata and sequences against a naive restatement of the two rules.  Every array holds exactly the entries the call
// may touch, so a read or write past an end is the sanitizer's to catch.  No GPU, no library: build with a host compiler
// under sanitizers and run:
//   c++ -std=c++17 -g -fsanitize=address,undefined -I kuiperllama_amd/csrc tools/lookup_fsm_draft_check.cpp -o lookup_fsm_draft_check
#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

#include "kh_lookup.h"

using Toks = std::vector<int32_t>;

struct Automaton {
  std::vector<int64_t> row_ptr{0};
  Toks tokens, next;
  void row(const std::map<int32_t, int32_t>& edges) {  // ascending by construction
    for (const auto& e : edges) tokens.push_back(e.first), next.push_back(e.second);
    row_ptr.push_back((int64_t)tokens.size());
  }
  kh_fsm view() const { return kh_fsm{(int32_t)row_ptr.size() - 1, 0, row_ptr.data(), tokens.data(), next.data()}; }
};
// the trie of the sequences, each followed by eos into a sink whose only edge is eos onto itself
static Automaton choices(const std::vector<Toks>& seqs, int32_t eos) {
  std::vector<std::map<int32_t, int32_t>> rows(1);
  std::vector<int> accepting;
  for (const Toks& q : seqs) {
    int s = 0;
    for (int32_t t : q) {
      if (!rows[(size_t)s].count(t)) {
        rows.emplace_back();
        rows[(size_t)s][t] = (int32_t)rows.size() - 1;
      }
      s = rows[(size_t)s][t];
    }
    accepting.push_back(s);
  }
  const int32_t sink = (int32_t)rows.size();
  rows.push_back({{eos, sink}});
  for (int s : accepting) rows[(size_t)s][eos] = sink;
  Automaton a;
  for (const auto& r : rows) a.row(r);
  return a;
}

struct Draft {
  Toks out;
  int forced;
  bool operator==(const Draft& o) const { return out == o.out && forced == o.forced; }
};
static Draft run(const Automaton& A, int32_t state, const Toks& seq, const Toks& hint, int hi, int lo, int cap) {
  const kh_fsm a = A.view();
  Toks out((size_t)cap), work(seq.size() + (size_t)cap);  // exactly what the call may touch
  int32_t forced = -1;
  const int n = kh_lookup_draft_fsm_core(&a, state, seq.empty() ? nullptr : seq.data(), (int)seq.size(),
                                         hint.empty() ? nullptr : hint.data(), (int)hint.size(), hi, lo,
                                         out.empty() ? nullptr : out.data(), cap, work.empty() ? nullptr : work.data(),
                                         &forced);
  if (n < 0 || n > cap || forced < 0 || forced > n) return std::printf("draft length %d / forced %d\n", n, forced), Draft{{-1}, -1};
  out.resize((size_t)n);
  return Draft{out, forced};
}
// the rules, word for word: a linear scan of the row, the n-gram drafter called on a copy of the text
static Draft naive(const Automaton& A, int32_t s, const Toks& seq, const Toks& hint, int hi, int lo, int cap) {
  auto edge = [&](int32_t st, int32_t t) -> int64_t {
    for (int64_t e = A.row_ptr[(size_t)st]; e < A.row_ptr[(size_t)st + 1]; ++e)
      if (A.tokens[(size_t)e] == t) return e;
    return -1;
  };
  Draft d{{}, 0};
  for (;;) {
    const size_t before = d.out.size();
    while ((int)d.out.size() < cap && A.row_ptr[(size_t)s + 1] - A.row_ptr[(size_t)s] == 1) {
      const int64_t e = A.row_ptr[(size_t)s];
      d.out.push_back(A.tokens[(size_t)e]);
      s = A.next[(size_t)e];
      ++d.forced;
    }
    const int room = cap - (int)d.out.size();
    if (room > 0) {
      Toks text(seq);
      text.insert(text.end(), d.out.begin(), d.out.end());
      Toks prop((size_t)room);
      const int n = kh_lookup_draft_core(text.empty() ? nullptr : text.data(), (int)text.size(),
                                         hint.empty() ? nullptr : hint.data(), (int)hint.size(), hi, lo, prop.data(), room);
      for (int i = 0; i < n; ++i) {
        const int64_t e = edge(s, prop[(size_t)i]);
        if (e < 0) break;
        d.out.push_back(prop[(size_t)i]);
        s = A.next[(size_t)e];
      }
    }
    if (d.out.size() == before || (int)d.out.size() >= cap) break;
  }
  return d;
}
// every drafted token is followable from the state the call was given
static bool followable(const Automaton& A, int32_t s, const Toks& out) {
  const kh_fsm a = A.view();
  for (int32_t t : out) {
    const int64_t e = kh_fsm_edge_host(&a, s, t);
    if (e < 0) return false;
    s = A.next[(size_t)e];
  }
  return true;
}

int main() {
  long checked = 0;
  bool ok = true;
  auto expect = [&](const Automaton& A, int32_t s, const Toks& seq, const Toks& hint, int hi, int lo, int cap,
                    const Draft& want) {
    const Draft got = run(A, s, seq, hint, hi, lo, cap);
    ++checked;
    if (got == want && naive(A, s, seq, hint, hi, lo, cap) == want && followable(A, s, got.out)) return true;
    std::printf("case %ld: %zu tokens drafted (%d forced), %zu (%d) expected\n", checked, got.out.size(), got.forced,
                want.out.size(), want.forced);
    return false;
  };
  const int32_t eos = 2;
  // a shared 2-token prefix and tails of 1, 6, 7 and 8 tokens
  std::vector<Toks> seqs;
  for (int n : {1, 6, 7, 8}) {
    Toks q{10, 11};
    for (int i = 0; i < n; ++i) q.push_back(100 * n + i);
    seqs.push_back(q);
  }
  const Automaton C4 = choices(seqs, eos);
  ok &= kh_fsm_check_host(nullptr, 2048) == KH_ERR_INVALID_ARG;
  {
    const kh_fsm a = C4.view();
    ok &= kh_fsm_check_host(&a, 2048) == KH_OK;
  }
  ok &= expect(C4, 0, {5}, {}, 4, 1, 7, {{10, 11}, 2});
  ok &= expect(C4, 0, {5}, {}, 4, 1, 1, {{10}, 1});
  ok &= expect(C4, 0, {5}, {}, 4, 1, 0, {{}, 0});
  ok &= expect(C4, 2, {5, 10, 11}, {}, 4, 1, 7, {{}, 0});  // the branching row
  auto walk = [&](const Automaton& A, const Toks& q) {
    const kh_fsm a = A.view();
    int32_t s = 0;
    for (int32_t t : q) s = A.next[(size_t)kh_fsm_edge_host(&a, s, t)];
    return s;
  };
  ok &= expect(C4, walk(C4, {10, 11, 800}), {800}, {}, 4, 1, 7, {{801, 802, 803, 804, 805, 806, 807}, 7});
  ok &= expect(C4, walk(C4, {10, 11, 700}), {700}, {}, 4, 1, 7, {{701, 702, 703, 704, 705, 706, eos}, 7});
  ok &= expect(C4, walk(C4, {10, 11, 600}), {600}, {}, 4, 1, 7, {{601, 602, 603, 604, 605, eos, eos}, 7});
  ok &= expect(C4, walk(C4, {10, 11, 100}), {100}, {}, 4, 1, 7, {{eos, eos, eos, eos, eos, eos, eos}, 7});
  ok &= expect(C4, 0, {5}, {10, 11, 600, 601, 602, 603, 604, 605}, 4, 1, 7, {{10, 11, 600, 601, 602, 603, 604}, 2});
  ok &= expect(C4, 0, {5}, {10, 11, 600, 77, 602}, 4, 1, 7, {{10, 11, 600, 601, 602, 603, 604}, 6});
  // a single choice: forced from the start into the sink, whose self-edge keeps the run going
  const Automaton C1 = choices({{4, 5, 6}}, eos);
  for (int cap : {0, 1, 3, 4, 7}) {
    Toks want{4, 5, 6, eos, eos, eos, eos};
    want.resize((size_t)cap);
    ok &= expect(C1, 0, {9}, {}, 4, 1, cap, {want, cap});
  }
  // a forced run, an n-gram stretch, a forced run - in one call
  {
    const int V = 2048;
    Automaton A;
    A.row({{5, 1}});
    A.row({{6, 2}});
    std::map<int32_t, int32_t> free2, free5;
    for (int v = 0; v < V; ++v) free2[v] = v == 9 ? 3 : 2, free5[v] = 5;
    A.row(free2);
    A.row({{12, 4}});
    A.row({{13, 5}});
    A.row(free5);
    const Toks seq{3, 1, 5, 6, 7, 8, 9, 40, 3, 1};
    ok &= expect(A, 0, seq, {}, 4, 1, 7, {{5, 6, 7, 8, 9, 12, 13}, 4});
    ok &= expect(A, 0, seq, {}, 4, 1, 6, {{5, 6, 7, 8, 9, 12}, 3});
    ok &= expect(A, 0, seq, {}, 4, 1, 8, {{5, 6, 7, 8, 9, 12, 13}, 4});
    ok &= expect(A, 0, seq, {}, 4, 1, 1, {{5}, 1});
    ok &= expect(A, 0, seq, {}, 4, 1, 0, {{}, 0});
  }
  // random automata over small alphabets, rows of 1 .. 4 edges, with and without a hint
  uint32_t x = 2468u;
  auto rnd = [&](uint32_t n) { return (x = x * 1664525u + 1013904223u, (x >> 8) % n); };
  long forced_seen = 0, cut_seen = 0;
  for (int it = 0; it < 4000 && ok; ++it) {
    const uint32_t k = 3 + rnd(4), ns = 2 + rnd(6);
    Automaton A;
    for (uint32_t s = 0; s < ns; ++s) {
      std::map<int32_t, int32_t> r;
      const uint32_t edges = 1 + rnd(it % 3 ? 3 : 1);  // every third automaton: forced rows only
      while (r.size() < edges && r.size() < k) r[(int32_t)rnd(k)] = (int32_t)rnd(ns);
      A.row(r);
    }
    Toks seq(1 + rnd(30)), hint(it % 2 ? 1 + rnd(20) : 0);
    for (auto& t : seq) t = (int32_t)rnd(k);
    for (auto& t : hint) t = (int32_t)rnd(k);
    const int lo = 1 + (int)rnd(3), hi = lo + (int)rnd(4), cap = (int)rnd(9);
    const int32_t s0 = (int32_t)rnd(ns);
    const Draft want = naive(A, s0, seq, hint, hi, lo, cap);
    forced_seen += want.forced;
    cut_seen += (int)want.out.size() < cap;
    ok &= expect(A, s0, seq, hint, hi, lo, cap, want);
  }
  ok &= forced_seen > 1000 && cut_seen > 500;  // the cases bite
  if (!ok) return 1;
  std::printf("lookup_fsm_draft_check: %ld drafts ok (%ld forced tokens, %ld drafts short of cap)\n", checked, forced_seen,
              cut_seen);
  return 0;
}
