// set_upload.h -- one transaction for replacing a set's device tables: reserve the new tables beside the old ones,
// enqueue their copies and fills, wait once.  After the first failure every later request does nothing, and finish()
// releases what the transaction reserved, nulls the caller's pointers and leaves the first failure's text as the last
// error; after a success the tables are the caller's.  A transaction destroyed without finish() unwinds the same way.
// No HIP header: the device calls come through a backend, so tests/cpp/set_upload_tests.cpp drives this with counters.
//
// Backend: struct { using Status = ...;                       // Status() is success; a failing call records its own text
//                   std::string &last_error();
//                   Status reserve(const char *who, void **p, uint64_t bytes, const char *tag);
//                   void release(void *p);
//                   Status copy(const char *who, const char *stage, void *dst, const void *src, uint64_t bytes);
//                   Status fill(const char *who, const char *stage, void *dst, int byte, uint64_t bytes);
//                   Status wait(const char *who, const char *stage); }
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

namespace gpe {

template <class Backend>
class SetUpload {
   public:
    using Status = typename Backend::Status;
    // stage: what a failing copy, fill or wait says behind `who` ("upload", "grid upload"; NULL: nothing)
    SetUpload(Backend be, const char *who, const char *stage = "upload") : be_(be), who_(who), stage_(stage) {}
    SetUpload(const SetUpload &) = delete;
    SetUpload &operator=(const SetUpload &) = delete;
    ~SetUpload() { if (!tables_.empty()) unwind(); }

    // *p = a new table of count elements; count 0 (an optional table the set does not need): none, *p stays as it is
    template <typename T>
    void reserve(T **p, uint64_t count, const char *tag)
    {
        if (st_ != Status() || count == 0) return;
        st_ = be_.reserve(who_, (void **)p, count * sizeof(T), tag);
        if (st_ == Status()) tables_.push_back((void **)p);
    }
    // count elements of src to dst; count 0: nothing
    template <typename T>
    void copy(void *dst, const T *src, uint64_t count)
    {
        if (st_ == Status() && count) st_ = be_.copy(who_, stage_, dst, src, count * sizeof(T));
    }
    void fill(void *dst, int byte, uint64_t bytes)
    {
        if (st_ == Status() && bytes) st_ = be_.fill(who_, stage_, dst, byte, bytes);
    }
    // Waits for the copies and fills (the host's arrays may go away afterwards).  The first failure's status, with its
    // text as the last error and nothing reserved left; else success, and the transaction forgets the tables.
    Status finish()
    {
        if (st_ == Status()) st_ = be_.wait(who_, stage_);
        if (st_ != Status()) unwind();
        tables_.clear();
        return st_;
    }

   private:
    void unwind()
    {
        const std::string why = be_.last_error();                      // (a guarded release may report damage of its own)
        for (void **p : tables_) { be_.release(*p); *p = nullptr; }
        tables_.clear();
        be_.last_error() = why;
    }
    Backend be_;
    const char *who_, *stage_;
    Status st_ = Status();
    std::vector<void **> tables_;
};

}  // namespace gpe
