// CPU check of csrc/rb2_round_plan.h (tests/test_round_plan.py): every combination of the switches and facts that decide a round's form, against the
// invariants the driver's `internal:` fatals and the audit counter's short-circuit enforce.  A program of its own: prints
// "ROUND PLAN OK points <n> lean2 <m> forked <f> lite <l>" and returns 0, or says what does not hold and returns 1.
#include <cstdio>
#include <cstdlib>
#include "rb2_round_plan.h"

static const int TS = 16;                                          // ts_max of the enumeration; tiles on both sides of it
static long g_points = 0, g_lean2 = 0, g_forked = 0, g_lite = 0;

static void fail(const char *what, const RoundKnobs &k, const CountFacts &f, const CountPlan &p)
{
	fprintf(stderr, "%s: steady_on %d lean %d audit %d fork %d dir %d verify %d compact %d ts_max %d debug %d | spec %d allow %d nranks %d sparse %d steady %d own %d nst %u n2 %llu"
			" -> form %d audit %d forked %d tail %d met %d n2 %llu\n", what, k.steady_on, k.lean, k.lean_audit, k.lean_fork, k.lean_dir, k.lean_verify, k.compact_ok, k.ts_max, k.debug,
			(int)f.spec, (int)f.allow_lean, f.nranks, (int)f.sparse, (int)f.known_steady, (int)f.own_stream, f.nst_ub, (unsigned long long)f.n_lean2,
			(int)p.form, (int)p.audit, (int)p.forked, (int)p.one_launch_tail, (int)p.met_stage2, (unsigned long long)p.n_lean2);
	exit(1);
}
#define REQUIRE(cond, what) do { if (!(cond)) fail(what, k, f, p); } while (0)

// one point of the count plan, and every merge that may follow it
static int check_point(const RoundKnobs &k, const CountFacts &f)
{
	const CountPlan p = count_plan(k, f);
	const bool lean = p.form == CountForm::Lean1 || p.form == CountForm::Lean2;
	++g_points;
	REQUIRE(p.one_launch_tail == (f.nst_ub < (unsigned)k.ts_max), "the one-launch tail");
	if (lean) REQUIRE(f.nranks == 1 && !f.sparse && !f.spec && f.known_steady && k.steady_on && f.allow_lean && k.lean > 0, "a lean count outside a steady dense round of one engine");
	if (!lean) REQUIRE(p.form == (f.spec ? CountForm::Spec : f.nranks > 1 ? CountForm::Rank : CountForm::Plain), "the form of a count that is not lean");
	if (f.nranks > 1) REQUIRE(!lean, "a lean count on a sharded rank");
	if (p.form == CountForm::Lean2) REQUIRE(!p.one_launch_tail && !p.audit && k.lean == 2, "stage 2 on the one-launch tail, or in an audit round");
	if (p.audit) REQUIRE(p.form == CountForm::Lean1 && k.lean == 2 && k.lean_audit > 0 && !p.one_launch_tail, "an audit round that is not a stage-1 round of a stage-2 handle");
	if (p.forked) REQUIRE(p.form == CountForm::Lean2 && f.own_stream && !k.lean_verify && !k.debug && k.lean_fork, "a forked round");
	if (p.form == CountForm::Lean2) REQUIRE(p.forked == fork_in_force(k, f.own_stream), "fork_in_force and a stage-2 round disagree");
	// the counter: it moves by one exactly where stage 2 could take the round and audits are on; met_stage2 says "could take"
	const bool eligible = p.form == CountForm::Lean2 || p.audit;
	REQUIRE(p.met_stage2 == eligible, "met_stage2");
	REQUIRE(p.n_lean2 == f.n_lean2 + ((eligible && k.lean_audit > 0) ? 1u : 0u), "the stage-2 counter");
	if (k.lean_audit == 0) REQUIRE(p.n_lean2 == f.n_lean2 && !p.audit, "the counter moved, or a round was audited, with RB2_LEAN_AUDIT=0");
	if (eligible && k.lean_audit > 0) REQUIRE(p.audit == (p.n_lean2 % (uint64_t)k.lean_audit == 0), "the audit cadence");
	if (lean_stage_in_force(k, p.met_stage2) == 2) REQUIRE(k.lean == 2 && p.met_stage2, "lean_stage_in_force");
	if (p.form == CountForm::Lean2) { ++g_lean2; REQUIRE(lean_stage_in_force(k, p.met_stage2) == 2, "a stage-2 round on a handle that reports stage 1"); }
	if (p.forked) ++g_forked;

	Counted c;
	c.set(p);
	REQUIRE(c.lean() == lean && c.forked == p.forked && c.audit == p.audit, "the count record");
	for (int bits = 0; bits < 8; ++bits) {
		const MergeFacts mf = { (bits & 1) != 0, f.nranks, (bits & 2) != 0, (bits & 4) != 0 };
		const MergePlan m = merge_plan(k, c, mf);
		REQUIRE(m.lean == lean && m.stage2 == (p.form == CountForm::Lean2) && m.audit == p.audit && m.forked == p.forked, "the merge does not follow the count");
		if (m.lite) REQUIRE(m.lean && m.compact_out && k.lean_dir, "a window directory outside a lean compact round");
		REQUIRE(m.lite == (m.lean && m.compact_out && k.lean_dir != 0), "lite");
		if (m.compact_out) REQUIRE(k.compact_ok && mf.more_rounds && !mf.plain_next && (mf.known_ae || mf.nranks == 1), "compact windows where another reader may meet them");
		REQUIRE(m.compact_out == (k.compact_ok && mf.more_rounds && !mf.plain_next && (mf.known_ae || mf.nranks == 1)), "compact_out");
		if (m.lite) ++g_lite;
	}
	// forgetting: what each operation leaves
	Counted d = c; d.round = 7; d.mark_setup(7, false, 3);
	d.forget_form();
	REQUIRE(!d.lean() && !d.forked && !d.audit && d.round == 7 && d.setup_done(7, false, 3), "forget_form");
	d.set(p); d.forget_count();
	REQUIRE(!d.lean() && !d.forked && d.round == Counted::NONE && d.setup_done(7, false, 3) && !d.setup_done(7, true, 3) && !d.setup_done(7, false, 4) && !d.setup_done(8, false, 3), "forget_count");
	d.set(p); d.forget_all();
	REQUIRE(!d.lean() && !d.forked && d.round == Counted::NONE && !d.setup_done(7, false, 3), "forget_all");
	return (p.form == CountForm::Lean2 ? 1 : 0) | (p.forked ? 2 : 0);
}

static void named(bool ok, const char *what) { if (!ok) { fprintf(stderr, "named case: %s\n", what); exit(1); } }

int main()
{
	static const int AUDITS[4] = { 0, 1, 2, 8 };
	for (int kb = 0; kb < 64; ++kb) for (int lean = 0; lean <= 2; ++lean) for (int ai = 0; ai < 4; ++ai) for (int tsm = 0; tsm < 2; ++tsm) {
		RoundKnobs k;
		k.steady_on = kb & 1; k.lean_fork = (kb >> 1) & 1; k.lean_dir = (kb >> 2) & 1; k.lean_verify = (kb >> 3) & 1; k.compact_ok = (kb >> 4) & 1; k.debug = (kb >> 5) & 1;
		k.lean = lean; k.lean_audit = AUDITS[ai]; k.ts_max = tsm ? TS : 0;
		for (int own = 0; own < 2; ++own) {
			int seen = 0;                                          // 1: some round was a stage-2 round, 2: some round forked
			for (int fb = 0; fb < 16; ++fb) for (int nranks = 1; nranks <= 2; ++nranks) for (unsigned nst = TS - 1; nst <= TS; ++nst) for (uint64_t n2 = 0; n2 <= 17; ++n2) {
				const CountFacts f = { (fb & 1) != 0, (fb & 2) != 0, nranks, (fb & 4) != 0, (fb & 8) != 0, own != 0, nst, n2 };
				seen |= check_point(k, f);
			}
			// a handle meets stage-2 rounds exactly when the switches allow any (with RB2_LEAN_AUDIT=1 every one of them is audited), and
			// fork_in_force is true exactly when some of them would fork
			const bool reach = k.steady_on && k.lean == 2 && k.lean_audit != 1;
			if (((seen & 1) != 0) != reach || ((seen & 2) != 0) != (reach && fork_in_force(k, own != 0))) {
				fprintf(stderr, "fork_in_force %d and the rounds met (%d) disagree: kb %d lean %d audit %d own %d\n", (int)fork_in_force(k, own != 0), seen, kb, lean, k.lean_audit, own); return 1; }
		}
	}
	// 64 consecutive rounds that stage 2 could take: exactly every k-th is an audit round, none with k = 0 (and the counter stays)
	for (int ai = 0; ai < 4; ++ai) for (uint64_t start = 0; start <= 17; ++start) {
		RoundKnobs k; k.ts_max = TS; k.lean_audit = AUDITS[ai];
		uint64_t n2 = start; int audits = 0;
		for (int i = 1; i <= 64; ++i) {
			const CountPlan p = count_plan(k, CountFacts{ false, true, 1, false, true, true, TS, n2 });
			const bool want = k.lean_audit > 0 && (start + (uint64_t)i) % (uint64_t)k.lean_audit == 0;
			if (p.audit != want || (p.form == CountForm::Lean2) == want || !p.met_stage2) { fprintf(stderr, "audit cadence: k %d start %llu round %d: audit %d\n", k.lean_audit, (unsigned long long)start, i, (int)p.audit); return 1; }
			audits += p.audit; n2 = p.n_lean2;
		}
		const uint64_t want_n2 = k.lean_audit ? start + 64 : start;
		const int want_audits = k.lean_audit ? (int)((start + 64) / (uint64_t)k.lean_audit - start / (uint64_t)k.lean_audit) : 0;
		if (n2 != want_n2 || audits != want_audits) { fprintf(stderr, "audit cadence: k %d start %llu: %d audits, counter %llu\n", k.lean_audit, (unsigned long long)start, audits, (unsigned long long)n2); return 1; }
	}
	{	// the defaults (ts_max: the handle sets TS_MAX; any value does here)
		RoundKnobs k; k.ts_max = TS;
		named(k.steady_on == 1 && k.lean == 2 && k.lean_audit == 8 && k.lean_fork == 1 && k.lean_dir == 1 && k.lean_verify == 0 && k.compact_ok == 1 && k.debug == 0, "the default switches");
		named(fork_in_force(k, true) && !fork_in_force(k, false) && lean_stage_in_force(k, true) == 2 && lean_stage_in_force(k, false) == 1, "the switches in force by default");
		Counted c;
		const CountPlan big = count_plan(k, CountFacts{ false, true, 1, false, true, true, TS, 0 });
		c.set(big);
		const MergePlan mid = merge_plan(k, c, MergeFacts{ true, 1, true, false }), last = merge_plan(k, c, MergeFacts{ true, 1, false, false });
		named(big.form == CountForm::Lean2 && big.forked && !big.audit && !big.one_launch_tail && big.n_lean2 == 1, "one engine, steady batch, many tiles: stage 2, forked");
		named(mid.lean && mid.stage2 && mid.forked && mid.compact_out && mid.lite, "... not the last round: compact, lite");
		named(last.lean && last.stage2 && last.forked && !last.compact_out && !last.lite, "... the last round: not compact, not lite");
		const CountPlan small = count_plan(k, CountFacts{ false, true, 1, false, true, true, TS - 1, 0 });
		named(small.form == CountForm::Lean1 && !small.forked && !small.audit && small.one_launch_tail && !small.met_stage2 && small.n_lean2 == 0, "few tiles: stage 1, not forked");
		const CountPlan before = count_plan(k, CountFacts{ false, true, 1, false, false, true, TS, 0 });
		named(before.form == CountForm::Plain && !before.forked, "before the device's report: a plain count");
		const CountPlan eighth = count_plan(k, CountFacts{ false, true, 1, false, true, true, TS, 7 });
		named(eighth.form == CountForm::Lean1 && eighth.audit && !eighth.forked && eighth.n_lean2 == 8, "the eighth eligible round is an audit round");
		for (int fb = 0; fb < 32; ++fb) {
			const CountPlan rk = count_plan(k, CountFacts{ false, (fb & 1) != 0, 2, (fb & 2) != 0, (fb & 4) != 0, (fb & 8) != 0, (fb & 16) ? (unsigned)TS : (unsigned)TS - 1, 3 });
			c.set(rk);
			named(rk.form == CountForm::Rank && !rk.forked && !rk.audit && rk.n_lean2 == 3 && !c.lean() && !merge_plan(k, c, MergeFacts{ true, 2, true, false }).lite, "a sharded rank: the rank form, never lean");
		}
		const CountPlan sp = count_plan(k, CountFacts{ true, true, 1, true, true, true, TS, 0 });
		named(sp.form == CountForm::Spec && !sp.forked, "behind an in-place round: the spec form");
	}
	printf("ROUND PLAN OK points %ld lean2 %ld forked %ld lite %ld\n", g_points, g_lean2, g_forked, g_lite);
	return 0;
}
