// The form of a dense BCR round ("the forms of a round"), decided once from the switches of the handle and what the host knows
// when it queues the round.  Plain C++, no device code, so that a CPU program can include it (tests/test_round_plan.py).  The driver (rb2_engine.hip:
// round_counts, round_merge) reads a plan and launches what it says; the stats calls that report "the switch in force" use the same predicates.
#pragma once
#include <cstdint>

/* the switches that decide a round's form (the handle holds them with the driver's other switches: Knobs, read_knobs) */
struct RoundKnobs {
	int steady_on = 1;      // RB2_STEADY=0: the device's report of a round of one-member groups is read, but no launch is dropped for it; no lean rounds either
	int lean = 2;           // RB2_STEADY_LEAN: 0 = off, 1 = on (k_sym writes no INS_E / INS_A), 2 = on and the round is counted from A alone where it can be (k_count_lean)
	int lean_audit = 8;     // RB2_LEAN_AUDIT: every lean_audit-th round that stage 2 could take is counted by k_sym as in stage 1; 0 = never
	int lean_fork = 1;      // RB2_LEAN_FORK=0: the counting tail of a stage-2 round stays on the handle's stream
	int lean_dir = 1;       // RB2_LEAN_DIR=0: every round writes the per-leaf directory
	int lean_verify = 0;    // RB2_LEAN_VERIFY=1 (tests): k_sym + k_tscan1 run beside k_count_lean, k_lean_compare counts the words that differ (batch_end: fatal)
	int compact_ok = 1;     // RB2_COMPACT=0: dense rounds always write plain (three-plane) windows
	int ts_max = 0;         // RB2_TS_MAX: batches with fewer string tiles run their counting tail in one single-block launch (k_tscan_setup); the handle's default is TS_MAX
	int debug = 0;          // RB2_HIP_DEBUG: a drain behind every kernel group
};
/* how the counting phase of a round is queued.  Spec: behind an in-place round whose verdict is still on its way (k_sym<.., SPLIT>); Rank: on a rank of a
 * sharded index (k_sym<STRIDE>); Lean1: k_sym<.., LEAN> writes no INS_E / INS_A; Lean2: k_count_lean in the place of k_sym and k_tscan1 */
enum class CountForm : uint8_t { Plain, Spec, Rank, Lean1, Lean2 };

/* the forked round: the counting tail of a stage-2 round runs on the side stream.  Never from a caller's stream; not with RB2_LEAN_VERIFY (k_sym<LEAN>
 * writes head flags into A, which k_merge reads beside it) and not with RB2_HIP_DEBUG (a drain per group) */
inline bool fork_in_force(const RoundKnobs &k, bool own_stream) { return k.lean_fork && own_stream && !k.lean_verify && !k.debug; }
/* the lean stage a handle runs: one that has only met the one-launch tail (met_stage2 false) runs stage 1 whatever the switch says */
inline int lean_stage_in_force(const RoundKnobs &k, bool met_stage2) { return (k.lean == 2 && !met_stage2) ? 1 : k.lean; }

/* spec: rides behind the in-place round in front of it; allow_lean = false: a round counted lean that is run in place after all is counted again with
 * INS_E / INS_A; sparse: the in-place layout; known_steady: the device has reported a round of one-member groups only; nst_ub: string tiles of the
 * batch; n_lean2: counting phases of this batch that stage 2 could take so far, audit rounds included */
struct CountFacts { bool spec, allow_lean; int nranks; bool sparse, known_steady, own_stream; unsigned nst_ub; uint64_t n_lean2; };
/* met_stage2: stage 2 could take this round (it took it, or audits it) -- the caller remembers it for lean_stage_in_force; n_lean2: the counter's new value */
struct CountPlan { CountForm form; bool audit, forked, one_launch_tail, met_stage2; uint64_t n_lean2; };
inline CountPlan count_plan(const RoundKnobs &k, const CountFacts &f)
{
	CountPlan p = { CountForm::Plain, false, false, f.nst_ub < (unsigned)k.ts_max, false, f.n_lean2 };
	// lean: the dense one-engine count of a batch the host knows steady (the in-place layout's k_part_sparse / k_merge_leaf need INS_E / INS_A)
	int lean = (f.allow_lean && !f.spec && f.nranks == 1 && !f.sparse && f.known_steady && k.steady_on) ? k.lean : 0;
	// stage 2 has the three-launch tail only (k_tscan_setup reads the records of a k_sym launch), and not in an audit round
	if (lean == 2 && p.one_launch_tail) lean = 1;
	if (lean == 2) p.met_stage2 = true;
	if (lean == 2 && k.lean_audit > 0 && ++p.n_lean2 % (uint64_t)k.lean_audit == 0) { lean = 1; p.audit = true; }
	p.forked = lean == 2 && fork_in_force(k, f.own_stream);
	p.form = f.spec ? CountForm::Spec : f.nranks > 1 ? CountForm::Rank : lean == 2 ? CountForm::Lean2 : lean ? CountForm::Lean1 : CountForm::Plain;
	return p;
}

/* The last counting phase queued.  round_merge follows THIS record, never known_steady: a round counted before the host heard the report holds
 * INS_E / INS_A and is merged from them. */
struct Counted {
	static constexpr uint64_t NONE = (uint64_t)-1;
	uint64_t round = NONE;          // round whose counting phase is queued ahead of its merge (behind an in-place round)
	CountForm form = CountForm::Plain;
	bool audit = false;             // Lean1 because the round is an audit round of stage 2
	bool forked = false;            // Lean2 and its counting tail was queued on the side stream
	uint64_t setup_round = NONE;    // round whose k_setup ran inside its counting phase ...
	bool setup_sparse = false; uint64_t setup_epoch = 0;   // ... for this layout, at this layout epoch (a re-layout in between: k_setup runs again)
	bool lean() const { return form == CountForm::Lean1 || form == CountForm::Lean2; }
	void set(const CountPlan &p) { form = p.form; audit = p.audit; forked = p.forked; }
	void mark_setup(uint64_t r, bool sparse, uint64_t epoch) { setup_round = r; setup_sparse = sparse; setup_epoch = epoch; }   // k_setup of round r is queued
	bool setup_done(uint64_t r, bool sparse, uint64_t epoch) const { return setup_round == r && setup_sparse == sparse && setup_epoch == epoch; }   // ... and still stands
	void forget_form() { form = CountForm::Plain; audit = forked = false; }   // the record belongs to a round that is merged, or counted again
	void forget_count() { round = NONE; forget_form(); }                       // what is queued ahead is counted again; its k_setup stands
	void forget_all() { setup_round = NONE; forget_count(); }                  // rounds were taken back
};

/* known_ae: the host can tell that every interval of the batch is empty; more_rounds: r < max_len -- the batch's last round leaves plain windows to
 * whoever reads the pool next; plain_next: a re-layout is pending, and it reads plain windows */
struct MergeFacts { bool known_ae; int nranks; bool more_rounds, plain_next; };
/* lean, stage2, audit, forked: how the round was counted.  compact_out: k_merge may write compact windows (only k_merge reads them again before the next
 * rewrite; one engine: the kernel itself checks that every interval is empty, a rank goes by the global flag).  lite: the new side keeps its rank
 * directory per window (k_merge<.., LITE>, k_meta_win, k_advance<.., LITE>) */
struct MergePlan { bool lean, stage2, audit, forked, compact_out, lite; };
inline MergePlan merge_plan(const RoundKnobs &k, const Counted &c, const MergeFacts &f)
{
	const bool compact_out = k.compact_ok && (f.known_ae || f.nranks == 1) && f.more_rounds && !f.plain_next;
	return { c.lean(), c.form == CountForm::Lean2, c.lean() && c.audit, c.forked, compact_out, c.lean() && compact_out && k.lean_dir != 0 };
}
