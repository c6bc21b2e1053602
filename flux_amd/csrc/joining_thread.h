// joining_thread.h -- a std::thread that is joined on every path out of its scope, unwinding included.  Destroying a joinable
// std::thread calls std::terminate, which inside a C-ABI call ends the client's process.  The thread's function must not throw:
// the builders catch what they throw and hand it back to the thread that joins them.
#pragma once
#include <thread>
#include <type_traits>
#include <utility>

namespace flux {

class JoiningThread {
  public:
    JoiningThread() = default;
    template <class F, class = std::enable_if_t<!std::is_same<std::decay_t<F>, JoiningThread>::value>>
    explicit JoiningThread(F &&f) : t_(std::forward<F>(f)) {}
    JoiningThread(JoiningThread &&) noexcept = default;
    JoiningThread &operator=(JoiningThread &&o) noexcept {
        join();
        t_ = std::move(o.t_);
        return *this;
    }
    ~JoiningThread() { join(); }
    void join() {
        if (t_.joinable()) t_.join();
    }

  private:
    std::thread t_;
};

}  // namespace flux
