/* Block runtime of cuda_on_cpu.h: a launch runs its blocks one after another, in blockIdx order (x fastest), and
 * a block's threads as ucontext fibers.  Between two barriers the live fibers run one at a time in thread-rank
 * order, each up to its next barrier or its return, so the whole run is single-threaded and deterministic: sums
 * that the kernels accumulate with atomicAdd are made in a fixed order and two runs give the same bits.  A thread
 * that has returned no longer takes part in barriers (a kernel whose threads leave before a barrier the others
 * still reach keeps running, as it does on the hardware the sources were written for). */
#include "cuda_on_cpu.h"

#include <ucontext.h>

#include <memory>

namespace cuda_on_cpu {

Indices current;

namespace {
const size_t STACK_BYTES = 256 * 1024; /* per fiber; the render kernels' frames are a few KiB */
const int MAX_THREADS = 1024;

ucontext_t scheduler, fiber[MAX_THREADS];
bool done[MAX_THREADS];
int running;                    /* rank of the fiber that runs */
int count_arriving, count_last; /* __syncthreads_count: predicates at the barrier being reached / just passed */
const std::function<void()> *body;
std::unique_ptr<char[]> stacks;
size_t stacks_for = 0;

void entry() {
    (*body)();
    done[running] = true;
    swapcontext(&fiber[running], &scheduler);
}

void run_block(dim3 block_index, dim3 grid, dim3 block, int n) {
    Indices idx[MAX_THREADS];
    for (int t = 0; t < n; t++) {
        done[t] = false;
        getcontext(&fiber[t]);
        fiber[t].uc_stack.ss_sp = stacks.get() + STACK_BYTES * t;
        fiber[t].uc_stack.ss_size = STACK_BYTES;
        fiber[t].uc_link = &scheduler;
        makecontext(&fiber[t], entry, 0);
        idx[t].thread = dim3(t % block.x, (t / block.x) % block.y, t / (block.x * block.y));
        idx[t].block = block_index;
        idx[t].block_dim = block;
        idx[t].grid_dim = grid;
    }
    count_last = 0;
    for (bool any = true; any;) {
        any = false;
        count_arriving = 0;
        for (int t = 0; t < n; t++) {
            if (done[t]) continue;
            running = t;
            current = idx[t];
            swapcontext(&scheduler, &fiber[t]);
            any = any || !done[t];
        }
        count_last = count_arriving;
    }
}
}  // namespace

void barrier() { swapcontext(&fiber[running], &scheduler); }

int barrier_count(int predicate) {
    count_arriving += predicate ? 1 : 0;
    barrier();
    return count_last;
}

void launch(const std::function<void()> &thread_body, dim3 grid, dim3 block) {
    const int n = (int)(block.x * block.y * block.z);
    if (n <= 0 || n > MAX_THREADS) {
        fprintf(stderr, "cuda_on_cpu: a block of %d threads\n", n);
        abort();
    }
    if (stacks_for < (size_t)n) { /* left uninitialised: pages are touched only as fibers use them */
        stacks.reset(new char[STACK_BYTES * n]);
        stacks_for = n;
    }
    body = &thread_body;
    for (unsigned bz = 0; bz < grid.z; bz++)
        for (unsigned by = 0; by < grid.y; by++)
            for (unsigned bx = 0; bx < grid.x; bx++) run_block(dim3(bx, by, bz), grid, block, n);
    body = nullptr;
}

}  // namespace cuda_on_cpu
