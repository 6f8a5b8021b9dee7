// Call scratch ("call scratch"): memory that lives for one API call.  CallScope owns what the call allocates and gives it
// back on every way out; Carve states the layout of a buffer with more than one tenant once.  Plain C++, no device code, so that a CPU program can
// include it (tests/test_scratch.py).  The includer defines rb2_fatal.
#pragma once
#include <cstddef>
#include <cstdint>

[[noreturn]] static void rb2_fatal(const char *fmt, ...);

/* make<B>() creates a B that the scope owns: any type with a release_quiet() that frees without reporting errors.  The destructor releases them in
 * reverse order of creation (a normal return, an exception unwinding).  The open scopes of a thread form a chain; release_open() -- rb2_fatal
 * calls it in front of a handler that may leave by longjmp or exit -- empties and unlinks them all, innermost first, so that destructors which
 * still run afterwards find nothing.  What make() returned is gone with it: nothing behind a release_open() may look at its call's scratch */
class CallScope {
	struct Item { Item *next = nullptr; virtual void drop() = 0; virtual ~Item() {} };
	template <class B> struct Held : Item { B b; void drop() override { b.release_quiet(); } };
	Item *items = nullptr;
	CallScope *prev;
	bool open = true;
	static CallScope *&head() { static thread_local CallScope *h = nullptr; return h; }
	void drop_all() { while (Item *i = items) { items = i->next; i->drop(); delete i; } }
public:
	CallScope() : prev(head()) { head() = this; }
	~CallScope() { drop_all(); if (open) head() = prev; }
	CallScope(const CallScope&) = delete;
	CallScope &operator=(const CallScope&) = delete;
	template <class B> B &make() { Held<B> *i = new Held<B>(); i->next = items; items = i; return i->b; }
	static void release_open() { while (CallScope *s = head()) { head() = s->prev; s->open = false; s->drop_all(); } }
};

/* take<T>(n) hands out the next region of n items and starts the one behind it at a multiple of 8 bytes; without a base it only counts.  size():
 * the bytes up to the end of the last region.  Sizes saturate at SAT instead of wrapping (an allocation of SAT bytes fails with its own message) */
class Carve {
	char *base;
	size_t off = 0, end = 0;
public:
	static constexpr size_t SAT = (SIZE_MAX / 2) & ~(size_t)7;
	explicit Carve(void *b = nullptr) : base((char*)b) {}
	template <class T> T *take(size_t n)
	{
		const size_t at = off;
		if (n > (SAT - at) / sizeof(T)) { off = end = SAT; return nullptr; }
		end = at + n * sizeof(T); off = (end + 7) & ~(size_t)7;
		return base ? (T*)(base + at) : nullptr;
	}
	size_t size() const { return end; }
};

/* buf (ensure(items), p) laid out by layout(Carve&): once counting, for the size, and behind the ensure on the buffer itself */
template <class Buf, class F> static void carve_in(Buf &buf, F layout)
{
	Carve count;
	layout(count);
	const size_t item = sizeof(*buf.p);
	buf.ensure(count.size() / item + (count.size() % item != 0));
	Carve real(buf.p);
	layout(real);
	if (real.size() != count.size()) { rb2_fatal("[rb2_hip] internal: a scratch layout takes %zu bytes where its counting pass said %zu\n", real.size(), count.size()); }
}
