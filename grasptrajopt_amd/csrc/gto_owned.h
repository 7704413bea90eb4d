// gto_owned.h — an allocation that frees itself: the owner of every device and pinned buffer behind the C ABI.
// gto_api.hip uses Owned<hipFree> and Owned<hipHostFree>.  The free function is a template argument, so this header needs
// no HIP header and the class is tested on the CPU with a counting fake (tests/owned_buffer_main.cpp).
//
// An owner lives in an object on the heap or on the stack (a handle, a scene's entry, an observation, a call's locals),
// NEVER in a static or global object: its destructor would call into the runtime while the process exits, when the runtime
// may be gone already.  The one process-wide cache of gto_api.hip, DepthPool, stays on raw pointers for that reason.
#ifndef GTO_OWNED_H
#define GTO_OWNED_H

#include <cstddef>
#include <utility>

template <auto Free>
class Owned {
 public:
  using Status = decltype(Free(static_cast<void*>(nullptr)));  // the runtime's error type; its zero value is success

  Owned() = default;
  Owned(void* p, size_t bytes) : p_(p), bytes_(bytes) {}  // takes over an allocation of `bytes` bytes
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  Owned(Owned&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      (void)reset();
      p_ = std::exchange(o.p_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  ~Owned() { (void)reset(); }

  // Frees now and says how it went; the owner is empty afterwards either way (a failed free is not tried again).
  Status reset() {
    Status s{};
    if (p_) s = Free(p_);
    p_ = nullptr;
    bytes_ = 0;
    return s;
  }

  void* get() const { return p_; }
  template <class T>
  T* as() const { return static_cast<T*>(p_); }
  size_t bytes() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

#endif  // GTO_OWNED_H
