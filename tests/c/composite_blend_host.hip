// composite_blend_host.hip -- hap_amd/csrc/composite_blend.hpp compiled for the host (hipcc --offload-host-only -shared):
// the definition's functions and the packed forms the kernel runs, over their whole domains, for
// tests/test_composite_blend_host.py.
#include <stddef.h>
#include <stdint.h>

#include "composite_blend.hpp"

using namespace hapbc::composite;

// out[x] = rdiv255(x), x = 0 .. 65025
extern "C" void composite_rdiv255(uint16_t *out)
{
    for (unsigned x = 0; x <= 65025u; x++)
        out[x] = (uint16_t)rdiv255(x);
}

// out[As << 8 | o] = a.  kernel_form: through layer_alpha_in_byte_2, the byte picked as the kernel's v_perm_b32 does
extern "C" void composite_layer_alpha(int kernel_form, uint16_t *out)
{
    for (unsigned As = 0; As < 256u; As++)
        for (unsigned o = 0; o < 256u; o++) {
            const unsigned m = layer_alpha_in_byte_2(As, opacity_scaled(o));
            // (nothing above byte 2: what the kernel's 24-bit multiply-add relies on)
            out[As << 8 | o] = (uint16_t)(kernel_form ? (m >> 24 ? 0xFFFFu : (m >> 16) & 0xFFu) : layer_alpha(As, o));
        }
}

// the kernel's pair, as it spreads a texel: lane 0 the colour, lane 1 the canvas's alpha (source 255)
static inline void pair(unsigned Cs, unsigned Cd, unsigned Ad, unsigned a, unsigned *colour, unsigned *alpha)
{
    const unsigned a2 = a | a << 16, inv2 = 0x00FF00FFu - a2;
    const unsigned r = as_dword(blend_pair(as_pk_u16(Cs | 255u << 16), as_pk_u16(Cd | Ad << 16), as_pk_u16(a2), as_pk_u16(inv2)));
    *colour = r & 0xFFFFu;
    *alpha = r >> 16;
}

// out[Cs << 16 | Cd << 8 | a] = Cd'.  (The kernel form's other lane carries the alpha of Ad = Cs: any byte will do.)
extern "C" void composite_blend_colour(int kernel_form, uint16_t *out)
{
    for (unsigned Cs = 0; Cs < 256u; Cs++)
        for (unsigned Cd = 0; Cd < 256u; Cd++)
            for (unsigned a = 0; a < 256u; a++) {
                unsigned colour = blend_colour(Cs, Cd, a), alpha;
                if (kernel_form)
                    pair(Cs, Cd, Cs, a, &colour, &alpha);
                out[Cs << 16 | Cd << 8 | a] = (uint16_t)colour;
            }
}

// out[Ad << 8 | a] = Ad'
extern "C" void composite_blend_alpha(int kernel_form, uint16_t *out)
{
    for (unsigned Ad = 0; Ad < 256u; Ad++)
        for (unsigned a = 0; a < 256u; a++) {
            unsigned colour, alpha = blend_alpha(Ad, a);
            if (kernel_form)
                pair(a, Ad, Ad, a, &colour, &alpha);
            out[Ad << 8 | a] = (uint16_t)alpha;
        }
}
