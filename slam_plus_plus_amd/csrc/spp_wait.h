// spp_wait.h -- the in-kernel hand-off through a word in device memory, once: the bounded wait, the release side, the
// acquire side. Device only.
//
// EVERY WAIT IS BOUNDED. A workgroup that polls a word another workgroup (or stream) will write cannot know that the
// writer still runs, and these machines are shared: a wait that never ends is a hung GPU. So every wait carries a
// WaitBound -- an abort word in device memory and a number of ticks of the 100 MHz wall clock -- and ends in one of three
// ways: the readiness test holds; the abort word says that somebody has given up already (nothing is stored); the
// wait's own clock bound is exceeded (the give-up value is stored into the abort word). From then on every other wait on
// that abort word falls through at its next bound check, so a launch drains within about one bound however many waits
// lie behind one another, and the host, which finds the word set, reports the failure and switches that context to the
// schedule without in-kernel waits (tail_disabled, sync_state = -1, sparse_dag_disable, chain_disabled). Progress without
// a timeout is each schedule's own argument (dispatch order: whatever a workgroup waits for is produced by workgroups
// dispatched before it that never wait for a later one); the bound is what holds when that argument or the machine fails.
//
// Polls are relaxed agent-scope loads inside the caller's readiness test (an acquire load would invalidate the L2 on every
// poll), each failed poll ends in s_sleep, and the abort word and the clock are looked at every EVERY-th failed poll only:
// both cost a poll's latency.
//
// Two kinds of abort word:
//   TAGGED = false  the word belongs to one launch or is zeroed by the host in front of it: any non-zero value is an abort.
//                   The clock starts in front of the first poll, the bound is checked on failed poll EVERY, 2 EVERY, ..
//   TAGGED = true   the word is never reset: `give_up` is a non-zero tag of this launch, a word equal to it is an abort,
//                   any other value is an earlier launch's and means nothing. The clock starts behind the first failed
//                   poll and the bound is checked on that poll already and on every EVERY-th after it, so a wait that is
//                   satisfied at once executes the readiness test alone, and a bound of one tick fires on the first
//                   failed poll (the load of the abort word lies between the two clock reads).
// The wait is per lane: one polling lane, a wave that polls as one (__all inside the readiness test) and divergent lanes
// that each poll a word of their own all work; lanes that give up store the same value.
#pragma once

namespace spp {

struct WaitBound {
	int *abort;      // abort word in device memory
	long long ticks; // bound of one wait, 100 MHz wall clock
};

__device__ __forceinline__ int wait_ld(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// true: ready() held. false: gave up (see above). ready() does its own relaxed loads and may leave what it read in the
// caller's variables.
template <int SLEEP, int EVERY, bool TAGGED = false, class Ready>
__device__ __forceinline__ bool bounded_wait(const WaitBound &wb, const int give_up, Ready ready)
{
	static_assert(EVERY > 0 && (EVERY & (EVERY - 1)) == 0, "the cadence is a power of two");
	long long t0 = TAGGED ? 0 : wall_clock64();
	for(int it = 0;; ++ it) {
		if(ready())
			return true;
		if(TAGGED && it == 0)
			t0 = wall_clock64();
		if((it & (EVERY - 1)) == (TAGGED ? 0 : EVERY - 1)) {
			const int ab = wait_ld(wb.abort);
			if(TAGGED ? ab == give_up : ab != 0)
				return false;
			if(wall_clock64() - t0 > wb.ticks) {
				__hip_atomic_store(wb.abort, give_up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				return false;
			}
		}
		__builtin_amdgcn_s_sleep(SLEEP);
	}
}

// ---- the release side: every storing wave has drained its stores, the workgroup barrier, then ONE lane makes them
// visible device-wide (agent-scope release, waited for) and runs `last`: the relaxed store or add that announces them
__device__ __forceinline__ void release_by_lane()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <class Last>
__device__ __forceinline__ void publish(Last last)
{
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	__syncthreads();
	if(threadIdx.x == 0) {
		release_by_lane();
		last();
	}
}

__device__ __forceinline__ void publish_store(int *flag, const int value)
{
	publish([&]() { __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
}

__device__ __forceinline__ void publish_add(int *counter)
{
	publish([&]() { __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
}

// ---- the acquire side: the lane that polled drops the stale lines and waits for that; the caller's barrier holds the
// other waves' loads behind it
__device__ __forceinline__ void acquire_by_lane()
{
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

} // namespace spp
