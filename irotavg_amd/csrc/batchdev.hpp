// batchdev.hpp -- the host's side of a batched call on the caller's packed device arrays, written once for the three
// families that have one (window.hip: the solve, wincov.hip: uncertainty and gate, winmst.hip: the initialisation).
// One object per family and process: a pinned, device-visible block [nb result records | nb descriptors] (batch_block,
// winbatch.hpp) that the workgroups read their problem from and leave their result in, the sequence number of the last
// call (hostwait.hpp) and a mutex that serialises the family's calls -- two families do not wait for each other.
//   stage   lock, block large enough and mapped for the CURRENT device, descriptors copied, every record's sequence
//           number cleared, a new number drawn
//   (the caller launches its kernels with Staged::D / Rd / seq)
//   finish  5 ms of polling (long batches, inputs still in flight on the caller's stream, a kernel that died), then the
//           stream is synchronised; the records in order; the first status that is not OK
// Rec has `int status, seq`; the lock goes with the Staged, also when a HIP call in between throws.
#pragma once
#include <cstring>
#include <mutex>

#include "common.hpp"    // MappedBlock, IRH_CHECK
#include "hostwait.hpp"  // next_seq, wait_seq
#include "winbatch.hpp"  // batch_block

namespace irh {

template <class Rec, class Desc>
struct BatchDev {
    static_assert(sizeof(Rec) % 8 == 0, "the descriptors behind the records hold 8-byte offsets");
    std::mutex mu;
    MappedBlock blk;  // portable: the callers' current devices may differ
    int seq = 0;

    struct Staged {
        std::unique_lock<std::mutex> lock;
        Rec *R;         // the records as the host sees them
        Rec *Rd;        // ... and as the current device does
        const Desc *D;  // the descriptors on the device
        int seq;
    };

    static BatchDev &get() {
        static BatchDev *w = new BatchDev();  // (created on first use, never destroyed: no HIP call at process exit)
        return *w;
    }

    Staged stage(const Desc *desc, size_t nb) {
        std::unique_lock<std::mutex> lock(mu);
        const BatchBlock L = batch_block(sizeof(Rec), sizeof(Desc), nb);
        blk.reserve(L.bytes, L.headroom, hipHostMallocPortable);
        blk.map();  // on every call: the current device can differ from the last call's
        Rec *R = reinterpret_cast<Rec *>(blk.host);
        std::memcpy(blk.host + L.oD, desc, sizeof(Desc) * nb);
        for (size_t b = 0; b < nb; b++) R[b].seq = 0;
        return Staged{std::move(lock), R, reinterpret_cast<Rec *>(blk.hdev), reinterpret_cast<const Desc *>(blk.hdev + L.oD),
                      next_seq(seq)};
    }

    // each(b, record b) in record order, once all of them show the call's sequence number
    template <class F>
    int finish(const Staged &s, hipStream_t stream, size_t nb, F &&each) {
        if (!wait_seq(&s.R[0].seq, sizeof(Rec), nb, s.seq, 5e-3)) IRH_CHECK(hipStreamSynchronize(stream));
        int rc = IROTAVG_OK;
        for (size_t b = 0; b < nb; b++) {
            if (s.R[b].status != IROTAVG_OK && rc == IROTAVG_OK) rc = s.R[b].status;
            each(b, s.R[b]);
        }
        return rc;
    }
};

}  // namespace irh
