// worker_driver.cpp -- host-only driver for `make tsan`: ThreadSanitizer over Worker (csrc/bsw_pool.h),
// the one-thread job queue behind the host pipeline's launcher and enqueuer (bsw_pipeline.hip).  No GPU.
//   - 1000 jobs from two producer threads are each handled once, in each producer's order
//   - stop() with jobs still queued handles all of them before it joins
//   - stop() on an idle worker, on one never started, and a second stop() return
//   - after a handler records an error, later jobs are still delivered -- what releases the
//     pipeline's finish(k) after a failed chunk -- and a waiter on the shared state sees each one
// Exit status 0 = every check passed (a ThreadSanitizer report ends the run).
#include <condition_variable>
#include <cstdio>
#include <mutex>
#include <thread>
#include <vector>
#include "../../bwa-mem2-arm_amd/csrc/bsw_pool.h"

static int g_fail = 0;
#define CHECK(c, ...)                                                    \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "CHECK failed %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                                \
            fprintf(stderr, "\n");                                       \
            ++g_fail;                                                    \
        }                                                                \
    } while (0)

struct Job { int producer = -1, seq = -1; };

static void test_two_producers()
{
    std::vector<Job> seen;                               // written by the worker thread only, read after stop()
    bool started = false;
    bsw::Worker<Job> w;
    w.start([&](Job &j) { seen.push_back(j); }, [&] { started = true; });
    auto produce = [&](int p) {
        for (int k = 0; k < 500; ++k) w.push(Job{p, k});
    };
    std::thread a(produce, 0), b(produce, 1);
    a.join();
    b.join();
    w.stop();
    CHECK(started, "on_start did not run");
    CHECK(seen.size() == 1000, "%zu of 1000 jobs handled", seen.size());
    int next[2] = {0, 0};
    for (const Job &j : seen) {
        CHECK(j.producer >= 0 && j.producer < 2 && j.seq == next[j.producer], "producer %d: job %d where %d was due",
              j.producer, j.seq, j.producer >= 0 && j.producer < 2 ? next[j.producer] : -1);
        if (j.producer >= 0 && j.producer < 2) ++next[j.producer];
    }
    CHECK(next[0] == 500 && next[1] == 500, "handled %d + %d jobs", next[0], next[1]);
}

static void test_stop_drains()
{
    std::mutex mu;
    std::condition_variable cv;
    bool open = false;                                   // closed: the handler blocks in its first job
    int handled = 0;
    bsw::Worker<Job> w;
    w.start([&](Job &) {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return open; });
        }
        ++handled;
    });
    for (int k = 0; k < 64; ++k) w.push(Job{0, k});      // (all but at most one still queued)
    {
        std::lock_guard<std::mutex> g(mu);
        open = true;
    }
    cv.notify_all();
    w.stop();
    CHECK(handled == 64, "stop() joined after %d of 64 queued jobs", handled);
}

static void test_idle_stop()
{
    {
        bsw::Worker<Job> w;
        w.start([](Job &) {});
        w.stop();
        w.stop();                                        // twice: nothing
    }
    {
        bsw::Worker<Job> never;                          // never started: stop() and the destructor return
        never.stop();
    }
    int handled = 0;
    {
        bsw::Worker<Job> w;                              // the destructor stops: queued jobs are handled
        w.start([&](Job &) { ++handled; });
        for (int k = 0; k < 10; ++k) w.push(Job{0, k});
    }
    CHECK(handled == 10, "destructor joined after %d of 10 jobs", handled);
}

// the pipeline's protocol in small: a first error under one mutex, a per-job `done` sequence a
// waiter blocks on; the handler skips the work of every job after an error but still marks it done
static void test_error_still_delivers()
{
    std::mutex mu;
    std::condition_variable cv;
    int err = 0, done = -1, worked = 0;
    bsw::Worker<Job> w;
    w.start([&](Job &j) {
        int r;
        {
            std::lock_guard<std::mutex> g(mu);
            r = err;
        }
        if (!r) {
            ++worked;
            if (j.seq == 3) r = -5;                     // the fourth job fails
        }
        {
            std::lock_guard<std::mutex> g(mu);
            if (r && !err) err = r;
            done = j.seq;
        }
        cv.notify_all();
    });
    for (int k = 0; k < 20; ++k) {
        w.push(Job{0, k});
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return done == k; });          // every job releases its waiter, failed or skipped
        CHECK((k < 3) == (err == 0), "job %d: error %d", k, err);
    }
    w.stop();
    CHECK(worked == 4 && err == -5 && done == 19, "worked %d, error %d, last done %d", worked, err, done);
}

int main()
{
    test_two_producers();
    test_stop_drains();
    test_idle_stop();
    test_error_still_delivers();
    printf("worker_driver: %s (%d failed checks)\n", g_fail ? "FAIL" : "ok", g_fail);
    return g_fail ? 1 : 0;
}
