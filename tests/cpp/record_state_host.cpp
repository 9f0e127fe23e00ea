// tests/cpp/record_state_host.cpp — taichi_mpm_amd/csrc/record_state.h (RecordState) on the host, header only.  rs_walk visits
// every state reachable from a fresh ctx under every transition with every argument value (seven booleans: at most 128 states,
// breadth first) and checks the invariants the host code relies on; the other scenarios replay the sequences of the host code that
// the invariants alone do not pin down.  Every scenario returns 0 or the line of the first check that failed;
// tests/test_record_state_cpu.py runs them.
#include "../../taichi_mpm_amd/csrc/record_state.h"

#include <cstddef>
#include <deque>

#define CHECK(cond) do { if (!(cond)) return __LINE__; } while (0)

namespace {
unsigned bits(const RecordState &s) {
  return (unsigned)s.sorted() | (unsigned)s.keys_valid() << 1 | (unsigned)s.pidc_valid() << 2 | (unsigned)s.affine_valid() << 3 |
         (unsigned)s.b_stale() << 4 | (unsigned)s.ordered() << 5 | (unsigned)s.compact() << 6;
}

enum Kind {
  PLAIN = 0,
  MOVES = 1,       // moves or replaces positions outside the G2P kernels: no index, key, id cache or record order survives
  NEEDS_B = 2,     // precondition !b_stale(): the callers run ensure_b_current() first
  MUST_CLEAR = 4,  // always asks for the block flags to be cleared
};
struct Transition {
  const char *name;
  int kind;
  bool (*apply)(RecordState &);  // what the transition returned (false for the void ones)
};
const Transition T[] = {
    {"records_dropped", MOVES | MUST_CLEAR, [](RecordState &s) { return s.records_dropped(); }},
    {"positions_changed", MOVES, [](RecordState &s) { return s.positions_changed(); }},
    {"particles_appended", MOVES | NEEDS_B, [](RecordState &s) { return s.particles_appended(); }},
    {"snapshot_loaded(false)", MOVES | MUST_CLEAR, [](RecordState &s) { return s.snapshot_loaded(false); }},
    {"snapshot_loaded(true)", MOVES | MUST_CLEAR, [](RecordState &s) { return s.snapshot_loaded(true); }},
    {"index_dropped", MOVES | MUST_CLEAR, [](RecordState &s) { return s.index_dropped(); }},
    {"affine_inputs_changed", NEEDS_B, [](RecordState &s) { s.affine_inputs_changed(); return false; }},
    {"ids_changed(false)", PLAIN, [](RecordState &s) { s.ids_changed(false); return false; }},
    {"ids_changed(true)", PLAIN, [](RecordState &s) { s.ids_changed(true); return false; }},
    {"id_cache_dropped", PLAIN, [](RecordState &s) { s.id_cache_dropped(); return false; }},
    {"sort_done", PLAIN, [](RecordState &s) { s.sort_done(); return false; }},
    {"reordered", PLAIN, [](RecordState &s) { s.reordered(); return false; }},
    {"affine_rebuilt", PLAIN, [](RecordState &s) { s.affine_rebuilt(); return false; }},
    {"b_recovered", PLAIN, [](RecordState &s) { s.b_recovered(); return false; }},
    {"g2p_done(false, false)", PLAIN, [](RecordState &s) { s.g2p_done(false, false); return false; }},
    {"g2p_done(false, true)", PLAIN, [](RecordState &s) { s.g2p_done(false, true); return false; }},
    {"g2p_done(true, false)", PLAIN, [](RecordState &s) { s.g2p_done(true, false); return false; }},
    {"g2p_done(true, true)", PLAIN, [](RecordState &s) { s.g2p_done(true, true); return false; }},
    {"records_swapped", PLAIN, [](RecordState &s) { s.records_swapped(); return false; }},
    {"records_imported", PLAIN, [](RecordState &s) { s.records_imported(); return false; }},
};
constexpr size_t NT = sizeof T / sizeof T[0];

int g_states = 0;  // states the last walk reached
}  // namespace

extern "C" {
int rs_transitions() { return (int)NT; }
int rs_states() { return g_states; }

int rs_walk() {
  bool seen[128] = {};
  std::deque<RecordState> todo;
  CHECK(bits(RecordState()) == 0);  // a fresh ctx: nothing is valid, nothing is stale
  seen[0] = true;
  todo.push_back(RecordState());
  g_states = 1;
  while (!todo.empty()) {
    const RecordState from = todo.front();
    todo.pop_front();
    for (size_t t = 0; t < NT; t++) {
      if ((T[t].kind & NEEDS_B) && from.b_stale()) continue;
      RecordState s = from;
      const bool clear = T[t].apply(s);
      CHECK(!(s.sorted() && s.keys_valid()));
      CHECK(!(s.pidc_valid() && !s.keys_valid()));
      CHECK(!(s.compact() && !s.ordered()));
      CHECK(!(s.b_stale() && !s.affine_valid()));
      if (T[t].kind & MOVES) {
        CHECK(!s.sorted() && !s.ordered() && !s.compact() && !s.pidc_valid() && !s.keys_valid());
        // the flags are cleared whenever the G2P kernels had set them for the old positions
        CHECK(clear || !from.keys_valid());
      }
      if (T[t].kind & MUST_CLEAR) CHECK(clear);
      if (!(T[t].kind & (MOVES | MUST_CLEAR))) CHECK(!clear);
      if (!seen[bits(s)]) {
        seen[bits(s)] = true;
        g_states++;
        todo.push_back(s);
      }
    }
  }
  // what the walk must have come through for the checks above to mean anything
  RecordState s;
  s.g2p_done(false, true);
  CHECK(seen[bits(s)]);  // keys + ids cached, A current, apic_b behind
  s.records_swapped();
  CHECK(seen[bits(s)]);
  s.sort_done();
  CHECK(seen[bits(s)]);
  return 0;
}

// ids_changed: the id cache goes in both modes; the sorted index only where its in-cell order is a function of the ids
int rs_ids_changed() {
  RecordState s;
  s.g2p_done(true, true);  // the state a G2P of the deterministic mode leaves: keys and ids ready for the next sort
  s.records_swapped();
  CHECK(s.keys_valid() && s.pidc_valid());
  s.ids_changed(true);
  CHECK(!s.pidc_valid() && !s.sorted());
  CHECK(s.keys_valid() && s.affine_valid() && s.ordered() && s.compact() && !s.b_stale());  // positions did not change
  for (int det = 0; det < 2; det++) {
    RecordState q;
    q.g2p_done(true, det != 0);
    q.sort_done();
    CHECK(q.sorted());
    q.ids_changed(det != 0);
    CHECK(!q.pidc_valid() && q.sorted() == (det == 0));
    CHECK(q.affine_valid() && !q.keys_valid());
  }
  return 0;
}

// one substep as do_sort / do_p2g / do_g2p / swap_records drive it, from fresh uploads, with apic_b kept and discarded
int rs_substep() {
  for (int store_b = 0; store_b < 2; store_b++)
    for (int det = 0; det < 2; det++) {
      RecordState s;
      CHECK(!s.particles_appended());  // nothing had set block flags
      CHECK(!s.keys_valid() && !s.affine_valid());
      s.sort_done();
      CHECK(s.sorted() && !s.ordered());
      s.affine_rebuilt();
      s.g2p_done(store_b != 0, det != 0);
      s.records_swapped();
      CHECK(!s.sorted() && s.keys_valid() && s.pidc_valid() == (det != 0) && s.affine_valid());
      CHECK(s.b_stale() == (store_b == 0) && s.ordered() && s.compact());
      s.sort_done();  // the next substep's sort reuses the keys: nothing but the index changes
      CHECK(s.sorted() && !s.keys_valid() && !s.pidc_valid() && s.ordered() && s.compact() && s.affine_valid());
      s.g2p_done(store_b != 0, det != 0);
      s.b_recovered();  // ensure_b_current, then an upload of F
      s.affine_inputs_changed();
      CHECK(!s.b_stale() && !s.affine_valid() && s.keys_valid());
      CHECK(s.positions_changed());  // upload of x: the G2P's flags must go
      CHECK(!s.positions_changed());  // ... once
      s.records_imported();
      CHECK(!s.compact());
    }
  return 0;
}

// dropping, loading and regrowing: what each leaves and whether it asks for the flags to be cleared
int rs_replace() {
  RecordState s;
  s.g2p_done(false, true);
  s.records_swapped();
  CHECK(s.records_dropped());
  CHECK(bits(s) == 0);
  CHECK(s.records_dropped());  // (k_import and the async kernels set flags without keys_valid: always cleared)
  CHECK(s.snapshot_loaded(true));  // (into a fresh ctx too: the load always clears, as a drop does)
  CHECK(s.affine_valid() && s.b_stale() && !s.keys_valid() && !s.sorted());
  s.b_recovered();
  s.g2p_done(true, true);
  s.records_swapped();
  CHECK(s.snapshot_loaded(false));  // over a ctx that had run: the old keys' flags go
  CHECK(s.affine_valid() && !s.b_stale() && !s.keys_valid() && !s.pidc_valid() && !s.ordered() && !s.compact());
  s.g2p_done(true, true);
  s.records_swapped();
  CHECK(s.index_dropped());
  CHECK(s.affine_valid() && !s.keys_valid() && !s.pidc_valid() && !s.sorted() && !s.ordered() && !s.compact());
  CHECK(s.index_dropped());
  s.g2p_done(true, true);
  s.id_cache_dropped();
  CHECK(!s.pidc_valid() && s.keys_valid());
  return 0;
}
}
