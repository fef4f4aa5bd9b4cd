// conv3_igemm_sres<..., M16> (unet_sres.h): the direct split-resident k3 conv kernel on v_mfma_f32_16x16x32_f16 tap pairs.  This file emits those
// instantiations and nothing else; unet_direct.hip decides when a launch takes them (option "m16") and emits the 32x32x16 half.
#include "unet_host.h"
#include "unet_sres.h"

namespace oai {

template <int RX, int RY, int WY, int WX>
void launch_sres_m16(int mrep, bool first, unsigned grid, hipStream_t st, const ConvArgs& a, const unsigned char* zero_rec) {
    if constexpr (RX == 16 && RY == 2 && WY == 4 && WX == 1) {
        if (first) {                                                 // ec0 fused into ec1's halo staging: the main shape only, 4 z slices per block
            conv3_igemm_sres<4, RX, RY, WY, WX, true, true><<<grid, 256, 0, st>>>(a, zero_rec);
            return;
        }
    }
    if (mrep == 4) conv3_igemm_sres<4, RX, RY, WY, WX, false, true><<<grid, 256, 0, st>>>(a, zero_rec);
    else conv3_igemm_sres<2, RX, RY, WY, WX, false, true><<<grid, 256, 0, st>>>(a, zero_rec);
}
// the block shapes of launch_conv3_direct (main, three x strips, two y strips); launch_conv3_one's face shapes are among them
template void launch_sres_m16<16, 2, 4, 1>(int, bool, unsigned, hipStream_t, const ConvArgs&, const unsigned char*);
template void launch_sres_m16<2, 16, 4, 1>(int, bool, unsigned, hipStream_t, const ConvArgs&, const unsigned char*);
template void launch_sres_m16<4, 8, 4, 1>(int, bool, unsigned, hipStream_t, const ConvArgs&, const unsigned char*);
template void launch_sres_m16<8, 4, 4, 1>(int, bool, unsigned, hipStream_t, const ConvArgs&, const unsigned char*);
template void launch_sres_m16<16, 2, 1, 4>(int, bool, unsigned, hipStream_t, const ConvArgs&, const unsigned char*);
template void launch_sres_m16<16, 2, 2, 2>(int, bool, unsigned, hipStream_t, const ConvArgs&, const unsigned char*);

}  // namespace oai
