// Host side of the front-end / back-end calls (include/NRDHip.h nrdHipPackInputs* / nrdHipResolveOutputs* / nrdHipPackShadowLights / nrdHipResolveShadowLights / nrdHipPackGuides), shared by their
// translation units: the kernels' view of a plane, the last error text and the checks every plane of a call goes through -- all of it in front of the first HIP call.
#pragma once

#include "NRD.h"
#include "NRDHip.h"

#include <cstdint>
#include <string>

namespace nrdhip {

struct FePlane { // 16 bytes of kernel argument per plane: every plane of a call has the same size
    uint8_t* ptr;
    uint32_t pitch;
};

inline thread_local std::string t_LastError; // nrdHipGetLastFrontEndError: one text per calling thread, shared by every front-end translation unit

inline uint32_t Fail(nrd::Result r, const std::string& text) {
    t_LastError = text;
    return (uint32_t)r;
}

inline uint32_t TexelBytes(nrd::Format f) {
    using F = nrd::Format;
    switch (f) {
        case F::R8_UNORM: case F::R8_UINT: return 1;
        case F::R16_UNORM: case F::R16_SFLOAT: return 2;
        case F::RGBA8_UNORM: case F::RGBA8_SNORM: case F::R10_G10_B10_A2_UNORM: case F::R32_SFLOAT: return 4;
        case F::RGBA16_UNORM: case F::RGBA16_SNORM: case F::RGBA16_SFLOAT: case F::RG32_SFLOAT: return 8;
        case F::RGB32_SFLOAT: return 12;
        case F::RGBA32_SFLOAT: return 16;
        default: return 0;
    }
}

// the checks of one call: every plane against the formats it may have and against the size of the first one seen
struct Checker {
    const char* entry;
    uint32_t result = (uint32_t)nrd::Result::SUCCESS;
    uint16_t w = 0, h = 0;
    // quarter-resolution calls (nrdHipPackInputsDecimated / nrdHipResolveOutputsUpsampled): a second size class. While `full` is set a plane is held against fw x fh, the
    // full-size planes of the call, instead of w x h, its low-size ones; once both are known, w x h must be ( ( fw + 1 ) >> 1 ) x ( ( fh + 1 ) >> 1 ). Never set by the other calls.
    uint16_t fw = 0, fh = 0;
    bool full = false;
    bool split = false;   // nrdHipPackInputsSplit / nrdHipResolveOutputsSplit: CheckColour accepts RGB32_SFLOAT
    uint32_t rgb = 0;     // kSplit* bits of the planes that hold it

    bool Failed() const { return result != (uint32_t)nrd::Result::SUCCESS; }
    void Error(nrd::Result r, const char* plane, const char* what) {
        if (!Failed())
            result = Fail(r, std::string(entry) + ": " + plane + ": " + what);
    }
    // required: says why the plane is needed (nullptr = optional); returns the kernel's view of the plane (ptr == nullptr: absent)
    FePlane Check(const NrdHipPlaneDesc& p, const char* name, const char* required, nrd::Format f0, nrd::Format f1 = nrd::Format::MAX_NUM) {
        FePlane out = {nullptr, 0};
        if (Failed())
            return out;
        if (!p.data) {
            if (required)
                Error(nrd::Result::INVALID_ARGUMENT, name, required);
            return out;
        }
        if (p.format != (uint32_t)f0 && (f1 == nrd::Format::MAX_NUM || p.format != (uint32_t)f1)) {
            Error(nrd::Result::UNSUPPORTED, name, "unexpected format");
            return out;
        }
        const uint32_t bpt = TexelBytes((nrd::Format)p.format);
        uint16_t &cw = full ? fw : w, &ch = full ? fh : h;
        if (!p.width || !p.height)
            Error(nrd::Result::INVALID_ARGUMENT, name, "empty plane");
        else if (cw && (p.width != cw || p.height != ch))
            Error(nrd::Result::INVALID_ARGUMENT, name, fw || full ? "size differs from the other planes of its size class (full-size / low-size) of the call" : "size differs from the other planes of the call");
        else if (bpt == 12u && ((p.rowPitchBytes % 4u) != 0 || ((uintptr_t)p.data % 4u) != 0)) // three packed dwords: dword alignment, rows need not start on a texel multiple
            Error(nrd::Result::INVALID_ARGUMENT, name, "row pitch or pointer of an RGB32_SFLOAT plane is not a multiple of 4");
        else if (bpt != 12u && ((p.rowPitchBytes % bpt) != 0 || ((uintptr_t)p.data % bpt) != 0))
            Error(nrd::Result::INVALID_ARGUMENT, name, "row pitch or pointer is not a multiple of the texel size");
        else if (p.rowPitchBytes < (uint32_t)p.width * bpt)
            Error(nrd::Result::INVALID_ARGUMENT, name, "row pitch below the row size");
        else if (!((uint64_t)p.rowPitchBytes < (1ull << 24) && (uint64_t)p.rowPitchBytes * p.height < (1ull << 32)))
            Error(nrd::Result::UNSUPPORTED, name, "row pitch >= 16 MiB or plane >= 4 GiB (planes are addressed with 32-bit byte offsets)");
        if (Failed())
            return out;
        cw = p.width;
        ch = p.height;
        if (w && fw && (w != ((fw + 1u) >> 1) || h != ((fh + 1u) >> 1))) {
            Error(nrd::Result::INVALID_ARGUMENT, name, "the low-size planes must be ( ( W + 1 ) >> 1 ) x ( ( H + 1 ) >> 1 ) of the W x H full-size planes");
            return out;
        }
        out.ptr = (uint8_t*)p.data;
        out.pitch = p.rowPitchBytes;
        return out;
    }
    // a plane documented as RGBA32_SFLOAT (f1: its other format, if any): the split calls take RGB32_SFLOAT as well and note it under `bit`; the old calls answer UNSUPPORTED as ever
    FePlane CheckColour(const NrdHipPlaneDesc& p, const char* name, const char* required, uint32_t bit, nrd::Format f1 = nrd::Format::MAX_NUM) {
        if (split && p.data && p.format == (uint32_t)nrd::Format::RGB32_SFLOAT) {
            const FePlane out = Check(p, name, required, nrd::Format::RGB32_SFLOAT);
            if (out.ptr)
                rgb |= bit;
            return out;
        }
        return Check(p, name, required, nrd::Format::RGBA32_SFLOAT, f1);
    }
    // the R32_SFLOAT plane `.w` of an RGB32_SFLOAT plane comes from / goes to: required next to RGB32_SFLOAT (when `required`), refused next to RGBA32_SFLOAT
    FePlane CheckCompanion(const NrdHipPlaneDesc& p, const char* name, bool ownerIsRgb, const char* required, const char* ownerName) {
        if (Failed())
            return FePlane{nullptr, 0};
        if (p.data && !ownerIsRgb) {
            Error(nrd::Result::INVALID_ARGUMENT, name, (std::string("given next to an RGBA32_SFLOAT ") + ownerName + ": .w would have two sources").c_str());
            return FePlane{nullptr, 0};
        }
        return ownerIsRgb ? Check(p, name, required, nrd::Format::R32_SFLOAT) : FePlane{nullptr, 0};
    }
};

// the planes checked while one of these lives belong to the full-size class (on = false: an ordinary call, nothing changes)
struct FullSize {
    Checker& c;
    FullSize(Checker& c_, bool on) : c(c_) { c.full = on; }
    ~FullSize() { c.full = false; }
};

// a plane the chosen mode or set of outputs has no use for must be absent: a caller who passes it expects something the call will not do
inline void Refuse(Checker& c, const NrdHipPlaneDesc& p, const char* name, const char* why) {
    if (p.data)
        c.Error(nrd::Result::INVALID_ARGUMENT, name, why);
}

inline bool IsRgb(const NrdHipPlaneDesc& p) { return p.format == (uint32_t)nrd::Format::RGB32_SFLOAT; }

// a layer stride of a plane the kernel reads `num` > 1 layers of; dwords: an RGB32_SFLOAT stack or an R32_SFLOAT companion (nrdHipPackInputsSplit)
inline void CheckLayerBytes(Checker& c, uint64_t layerBytes, const FePlane& plane, uint32_t num, const char* field, bool dwords = false) {
    if (c.Failed() || num <= 1u || !plane.ptr)
        return;
    if (dwords && layerBytes % 4u)
        c.Error(nrd::Result::INVALID_ARGUMENT, field, "the layer stride is not a multiple of 4");
    else if (!dwords && layerBytes % 16u)
        c.Error(nrd::Result::INVALID_ARGUMENT, field, "the layer stride is not a multiple of 16 (the texel size)");
    else if (layerBytes < (uint64_t)plane.pitch * c.h)
        c.Error(nrd::Result::INVALID_ARGUMENT, field, "the layer stride is below rowPitchBytes x height of the plane");
}

} // namespace nrdhip
