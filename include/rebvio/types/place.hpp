// Place recognition: EdgeMap::placeSignature, PlaceDb, Rebvio::setPlaceRecognition. No reference counterpart; include/rebvio_hip.h
// ("Place recognition") defines every term. PlaceMatch is layout-compatible with the C-ABI's rebvio_hip_place_match.
#pragma once

#include <array>
#include <cstdint>

namespace rebvio {
namespace types {

constexpr int kPlaceWords = 384;    // 8 x 6 image cells x 8 orientation bins
constexpr int kPlaceTopKMax = 16;   // the most matches one query returns
constexpr uint32_t kPlaceMaxDistance = 384u * 65535u;

using PlaceSignature = std::array<uint16_t, kPlaceWords>;

struct PlaceMatch {
  uint32_t distance{0};  // sum over the 384 words of |a[k] - b[k]|
  int32_t index{-1};     // the entry's row in the database
  uint64_t tag{0};       // as given when the entry was added (Rebvio: the keyframe's stamp, microseconds)
};
static_assert(sizeof(PlaceMatch) == 16, "PlaceMatch must stay layout-compatible with rebvio_hip_place_match");

}  // namespace types
}  // namespace rebvio
