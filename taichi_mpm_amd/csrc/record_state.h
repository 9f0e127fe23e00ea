// taichi_mpm_amd/csrc/record_state.h — which of mpmhip_ctx's particle arrays describe the current particles (host only: no HIP
// header, nothing launched, no stream; tests/test_record_state_cpu.py walks every reachable state with plain g++)
// The seven flags are private: the host code reads them through the getters and changes them through one named transition per
// thing that happens to the arrays.  A transition after which stale block flags could leak into the next sort (k_build_keys only
// ORs new flags on top: stale ones would become phantom active blocks) returns true; clear_block_flags() in mpmhip.hip turns that
// into the memset.
//
// Invariants over every reachable state (checked by the walk):
//   sorted     => !keys_valid   after a sort key[] holds k_rank's packed (rank, cell index) words
//   pidc_valid => keys_valid    pidc[] is only ever written together with key[]
//   compact    => ordered
//   b_stale    => affine_valid  apic_b is recovered FROM RecP.A (ensure_b_current)
// and after a transition that moves or replaces positions outside the G2P kernels (the first group below) none of sorted,
// keys_valid, pidc_valid, ordered, compact holds.
// b_stale => affine_valid rests on a precondition the transitions cannot see: affine_inputs_changed() and particles_appended()
// need !b_stale(), their callers run ensure_b_current() first.
// While k_build_keys has run and the sort's other kernels have not, pidc[] is current although keys_valid is false: do_sort holds
// that fact in a local, it is never a state of the ctx.
#pragma once

class RecordState {
 public:
  bool sorted() const { return sorted_; }              // perm / cell_start describe the current positions
  bool keys_valid() const { return keys_valid_; }      // key[] + block flags describe the current positions (written by the G2P kernels)
  bool pidc_valid() const { return pidc_valid_; }      // ... and pidc[] was written together with that key[] (every key writer does while Params::pidc is set)
  bool affine_valid() const { return affine_valid_; }  // RecP.A matches (F, aux, apic_b, dt)
  bool b_stale() const { return b_stale_; }            // discard_apic_b: the side array is behind RecP.A (the G2P kernels did not write it)
  bool ordered() const { return ordered_; }            // the records lie in the order of the last sort
  bool compact() const { return compact_; }            // ... and the live ones occupy exactly [0, cnt->n_sorted): n_slots may shrink to that

  // every record was dropped or replaced by others (clear, the async stepper's working sets and views): nothing describes them.
  // The flags are cleared whatever keys_valid says: k_import and the async kernels set block flags without it.
  [[nodiscard]] bool records_dropped() { *this = RecordState(); return true; }
  // positions changed outside the G2P kernels (upload of x / v, deletions): key[], pidc[], perm / cell_start and the record order
  // speak of the old ones.  True when key[] was current, i.e. when its block flags are set.
  [[nodiscard]] bool positions_changed() {
    const bool flags_set = keys_valid_;
    sorted_ = keys_valid_ = pidc_valid_ = ordered_ = compact_ = false;
    return flags_set;
  }
  // records were added behind the last slot: their RecP.A is not built yet, and positions_changed().  Needs !b_stale().
  [[nodiscard]] bool particles_appended() { affine_valid_ = false; return positions_changed(); }
  // the records of a snapshot replaced all others: records_dropped(), but RecP.A travels in the records; apic_b is current only
  // if the saving ctx kept it
  [[nodiscard]] bool snapshot_loaded(bool b_stale) {
    *this = RecordState();
    affine_valid_ = true; b_stale_ = b_stale;
    return true;
  }
  // key[], pidc[], rank[] and perm[] were reallocated without their contents (reserve); the records stay
  [[nodiscard]] bool index_dropped() { (void)positions_changed(); return true; }

  // F, aux, apic_b or dt changed: RecP.A no longer matches.  Needs !b_stale().
  void affine_inputs_changed() { affine_valid_ = false; }
  // RecG.pid was rewritten: pidc[] holds the old ids; in the deterministic mode the sorted index's in-cell order is a function of
  // the ids, so perm is behind too.  (The default mode reads neither pidc[] nor the ids: sorted stays.)
  void ids_changed(bool deterministic) { pidc_valid_ = false; if (deterministic) sorted_ = false; }
  // Params::pidc was switched on or off (set_deterministic): the key writers since the last G2P may not have written pidc[]
  void id_cache_dropped() { pidc_valid_ = false; }

  // perm / cell_start were built from key[] (and pidc[]), which the sort's kernels overwrote on the way
  void sort_done() { sorted_ = true; keys_valid_ = pidc_valid_ = false; }
  // the records were gathered into the order of the sort (do_reorder)
  void reordered() { ordered_ = true; }
  // k_affine rebuilt RecP.A from (F, aux, apic_b)
  void affine_rebuilt() { affine_valid_ = true; }
  // k_recover_b rebuilt apic_b from RecP.A
  void b_recovered() { b_stale_ = false; }
  // a G2P kernel moved the particles and wrote, for the next substep, key[] + block flags (pidc[] beside them: with_ids), RecP.A
  // and, when the ctx keeps it (store_b), apic_b
  void g2p_done(bool store_b, bool with_ids) {
    sorted_ = false; keys_valid_ = true; pidc_valid_ = with_ids; affine_valid_ = true;
    if (!store_b) b_stale_ = true;
  }
  // the buffers the last G2P launch of a substep wrote (records at their sorted positions, live ones first) became the records
  void records_swapped() { ordered_ = compact_ = true; }
  // k_import appended records (with their keys and block flags): live records now also sit behind the range G2P compacted
  void records_imported() { compact_ = false; }

 private:
  bool sorted_ = false, keys_valid_ = false, pidc_valid_ = false, affine_valid_ = false, b_stale_ = false, ordered_ = false,
       compact_ = false;
};
