"""The shared expressions and device pieces of csrc/ are written once (csrc/bn_expr.h, csrc/device.h).

Reads only the sources; no GPU, no build.  A kernel that recomputes a BatchNorm or activation pass calls the helpers of bn_expr.h:
several fusions rest on different kernels computing the same bits for the same expression, and a second spelling of one of
them is the start of two kernels that disagree.

A site that has to stay spelled out -- routed through the helper the kernel's device code differs from the parent build's
(tools/devcode_ab.py) -- is an entry of SPELLED_OUT with its reason, and carries a comment in the source.

The same for the host side of the kernel tries: the window origin, the tap tables relative to it, the extent of a
buffer descriptor, the dynamic-LDS opt-in, the whole-output gate and the declined status are in common.h only (LAUNCH_SPELLED_OUT).
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'segmentation-networks-benchmark_amd', 'csrc')

# (file, text of the site) -> why it is not routed through the shared helper
SPELLED_OUT = {
    ('wgrad_s1.hip', 'k_c2[e] = a.bna.bcoef[2 * a.bna.Cp + cch];'):
        'seven-constant load of conv_wgrad_s1x9_kernel BNA: through a shared loader (struct, by value, by reference) the '
        'compiler swaps the operands of the packed multiplies of the recompute',
    ('wgrad_roll.hip', 'k_c2[e] = a.tfd_bcoef[2 * a.tfd_Cp + c];'):
        'seven-constant load of conv_wgrad_c8roll_kernel TFD = 3: the same loader changes its register allocation',
    ('wgrad_roll.hip', 'd = __uint_as_float(pack2bf(d, 0.f) << 16);'):
        'bf16 rounding of conv_wgrad_c8roll_kernel TFD = 3 through the packed conversion: round_bf16 compiles to other code there',
}


def sources():
    out = {}
    for p in sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h'))):
        with open(p) as f:
            out[os.path.basename(p)] = f.read()
    assert len(out) > 20, 'csrc/ not found'
    return out


def files_with(pattern, src=None):
    src = src or sources()
    return {n: len(re.findall(pattern, t)) for n, t in src.items() if re.search(pattern, t)}


def test_negative_scale_ternary_is_written_once():
    # act == RELU ? 0 : (act == LEAKY ? slope : 1), under any operand names
    hits = files_with(r'==\s*SEGNB_ACT_RELU\s*\?\s*0\.f\s*:\s*\(?\s*[\w.\->]+\s*==\s*SEGNB_ACT_LEAKY')
    assert hits == {'bn_expr.h': 1}, hits


def test_dependent_one_liners_are_written_once():
    src = sources()
    # the scaled-negative forward of the activation epilogues: v < 0 ? v * neg + 0 : v
    assert files_with(r'<\s*0\.f\s*\?\s*\w+\s*\*\s*\w+\s*\+\s*0\.f\s*:', src) == {'bn_expr.h': 1}
    assert files_with(r'if\s*\(\w+\s*<\s*0\.f\)\s*\w+\s*=\s*\w+\s*\*\s*\w+\s*\+\s*0\.f', src) == {}
    # act'(z) with the hoisted scale: z > 0 ? 1 : neg
    assert files_with(r'>\s*0\.f\s*\?\s*1\.f\s*:\s*\w*neg\b', src) == {'bn_expr.h': 1}
    # the written-out bf16 rounding beside round_bf16
    assert files_with(r'bf16_bits_to_f32\(\s*f32_to_bf16_bits\(', src) == {'common.h': 1}


def test_helpers_are_defined_once():
    src = sources()
    for name in ('act_neg_scale', 'act_fwd', 'act_grad', 'act_fwd_neg', 'act_grad_neg', 'act_bwd_neg', 'bn_apply_elem',
                 'bn_fold5_row', 'round_bf16', 'xcd_remap', 'make_rsrc', 'make_rsrc4', 'unpack8', 'relu_pk2bf', 'lds_const8'):
        hits = files_with(r'__forceinline__\s+[\w:<>]+\s+%s\s*\(' % name, src)
        assert sum(hits.values()) == 1, (name, hits)
    # bn_dz_elem: the (act, slope) form and the form with the scale taken once, both in the header
    assert files_with(r'__forceinline__\s+float\s+bn_dz_elem\s*\(', src) == {'bn_expr.h': 2}
    for name in ('u32x4_t', 'u32x2_t', 'bf16x4_t', 'f32x4_t', 's16x2_t', 'i32x4_t', 'lds_bf16x4_ptr', 'lds_u8_ptr'):
        hits = files_with(r'typedef[^;\n]*\b%s;' % name, src)
        assert hits == {'device.h': 1}, (name, hits)


def test_suffixed_copies_are_gone():
    for name in ('xcd_remap_s1', 'xcd_remap_fd', 'unpack8w', 'relu_pk2bfw', 'lds_const8w', 's16x2w_t', 'wg_round_bf16',
                 'mu32x4_t', 'lds_bf16x4_t'):
        assert files_with(r'\b%s\b' % name) == {}, name


def test_descriptor_word_is_named_once():
    assert files_with(r'0x00020000') == {'device.h': 1}
    # ... and the builtin is wrapped once
    assert files_with(r'__builtin_amdgcn_make_buffer_rsrc') == {'device.h': 1}


def test_host_epilogue_setup_is_written_once():
    src = sources()
    # the y extent check with the seven field copies (conv_igemm.hip's general kernel has no descriptor over y: not this block)
    assert files_with(r'\.bn_y_bytes\s*=', src) == {'common.h': 1}
    assert files_with(r'\.ep_slope\s*=\s*ep\s*!=', src) == {'common.h': 1}
    for name in ('take_bn_reduce', 'take_act_epilogue'):
        assert sum(files_with(r'inline\s+\w+\s+%s\s*\(' % name, src).values()) == 1, name


def test_spelled_out_sites_are_the_listed_ones():
    src = sources()
    for (name, text), reason in SPELLED_OUT.items():
        assert reason
        assert src[name].count(text) == 1, (name, text)
        # the site says so itself: a comment in front of its loop or on its own line
        at = src[name].index(text)
        before = src[name][:at].split('\n')[-13:] + [src[name][at:].split('\n')[0]]
        assert any('//' in l and ('spelled out' in l or 'round_bf16' in l) for l in before), (name, text)
    # nothing else restates them: the seven-constant chunk load, and a bf16 rounding through pack2bf
    loads = files_with(r'\[e\]\s*=\s*[\w.\->]*bcoef\[2\s*\*', src)
    assert loads == {'wgrad_s1.hip': 1, 'wgrad_roll.hip': 1}, loads
    assert files_with(r'pack2bf\(\w+,\s*0\.f\)\s*<<\s*16', src) == {'wgrad_roll.hip': 1}


# ---- conv_fprop_ws_kernel's 16x16x32 matrix stream: one tap body and one staging for both row orders ---------
def _count(name, needle, src=None):
    """occurrences of the literal text in one file, without the sites listed in SPELLED_OUT / LAUNCH_SPELLED_OUT"""
    n = (src or sources())[name].count(needle)
    for table in (SPELLED_OUT, LAUNCH_SPELLED_OUT):
        for (f, text), reason in table.items():
            assert reason
            if f == name and needle in text:
                n -= 1
    return n


def test_ws_stream_has_one_tap_body_and_one_staging():
    src = sources()
    # the tap: the plain order and WsEpi call one lambda, so each MFMA macro of the 16x16x32 form has one call site
    assert _count('fprop_dma.hip', 'FD_MFMA16_0(', src) == 1
    assert _count('fprop_dma.hip', 'FD_MFMA16(', src) == 1
    # the staging: the MASK bit selection is written once (mb & 1u ... mask_neg, two lines of four selects)
    assert len(re.findall(r'\(mb & 1u\)[^\n]*mask_neg', src['fprop_dma.hip'])) == 1
    assert _count('fprop_dma.hip', 'mb & 1u', src) == 1 and _count('fprop_dma.hip', 'mb & 4u', src) == 1
    # a store row's address, store and statistics: row_store_of only (the per-gap row_step is gone)
    assert _count('fprop_dma.hip', '__builtin_amdgcn_raw_buffer_store_b128(v, rs_out', src) == 1
    assert files_with(r'\brow_step\s*=\s*\[', src) == {} and files_with(r'\bepi_tap\b', src) == {}


def test_whole_file_experiment_switches_are_gone():
    assert files_with(r'SEGNB_EXP') == {}


def test_ws_tile_grid_is_set_up_once():
    src = sources()
    dma, sel = src['fprop_dma.hip'], src['ws_select.h']
    # the persistent blocks per channel tile -- the division of the CUs, in ws_select.h's ws_blocks -- and their clamp to the tile count
    assert files_with(r'\bcus\s*/\s*ntl\b', src) == {'ws_select.h': 1}
    assert files_with(r'segnb_knob_conv_cus\(\)\s*/', src).get('fprop_dma.hip') is None
    assert len(re.findall(r'\bws_blocks\(cus, ntl\)', dma)) == 1
    assert _count('fprop_dma.hip', 'if (gm > a.IT) gm = a.IT;', src) == 1
    assert len(re.findall(r'a\.HB\s*=', dma)) == 1 and len(re.findall(r'a\.WB\s*=', dma)) == 1
    # ws_tile_div: defined once, called by the one grid helper
    assert len(re.findall(r'\bws_tile_div\(a\)', dma)) == 1
    # the mask / no statistics / timing / plain / split-K ladder: every instantiation form is named once (ws_form_kernel), taken
    # into a row's kernel table from the forms ws_select.h lists, and launched from the one site that indexes that table
    for form in ('<K, false>', '<K, false, false, false>', '<K, false, false, true, false, true>', '<K, false, true, false>', '<K, true>',
                 '<K, false, false, true, true>', '<K, false, false, false, true>'):
        assert _count('fprop_dma.hip', 'return conv_fprop_ws_kernel%s;' % form, src) == 1, form
    host = dma[dma.index('int ksplit_workspace('):]
    assert len(re.findall(r'conv_fprop_ws_kernel<', host)) == 7
    assert len(re.findall(r'hipLaunchKernelGGL\(', dma)) == 1 and 'hipLaunchKernelGGL(kern, ' in dma
    assert len(re.findall(r'segnb_opt_in_lds\(', dma)) == 1
    # ... and in fprop_rw.hip: a row's three forms once, the opt-in and the launch both from that list
    rw = src['fprop_rw.hip']
    assert len(re.findall(r'conv_fprop_rw_kernel<', rw)) == 3 and len(re.findall(r'hipLaunchKernelGGL\(', rw)) == 1
    assert len(re.findall(r'segnb_opt_in_lds\(', rw)) == 1
    # the round arithmetic -- tiles over persistent blocks, rounded up -- occurs in ws_select.h only
    assert files_with(r'\+\s*gm\s*-\s*1\)\s*/\s*gm', src) == {'ws_select.h': 1}
    assert not re.search(r'\bit[01]\b', dma) and not re.search(r'\bit[01]\b', rw)
    # one argument setup per file
    assert len(re.findall(r'\.x_bytes\s*=', dma)) == 1 and len(re.findall(r'\.x_bytes\s*=', rw)) == 1
    assert len(re.findall(r'\bWsArgs a\{\};', dma)) == 2 and len(re.findall(r'\bWsArgs a;', dma)) == 0       # (the two tries)
    assert len(re.findall(r'\bFdArgs a\{\};', rw)) == 1 and len(re.findall(r'\bFdArgs a;', rw)) == 0
    # the two closed switches are gone
    assert files_with(r'fprop_mf16|FPROP_MF16|rw_store_waves', src) == {}
    # ws_select.h is plain C++: no HIP, no knob, no allocation
    assert not re.search(r'#include\s*[<"](hip|common|device)|segnb_knob_|\bnew\b|malloc|std::(vector|function|string)', sel)


# ---- the host side of the kernel tries: window origin, descriptor extents, LDS opt-in, declined status --------
# (file, text of the site) -> why the site is not routed through the helper of common.h; none so far
LAUNCH_SPELLED_OUT = {}


def _elsewhere(pattern, src=None):
    """files other than common.h in which the pattern occurs, without the listed exceptions"""
    hits = files_with(pattern, src)
    hits.pop('common.h', None)
    for (name, text), reason in LAUNCH_SPELLED_OUT.items():
        assert reason
        if name in hits and re.search(pattern, text):
            hits[name] -= 1
    return {n: c for n, c in hits.items() if c}


def test_tap_window_is_computed_in_one_place():
    src = sources()
    # the window origin loop, under any names of the two minima, and the "each of the nine positions once" table
    assert files_with(r'\w*min\s*=\s*g->dh\[0\]', src).get('common.h') == 1
    assert _elsewhere(r'\w*min\s*=\s*g->dh\[0\]', src) == {}
    assert files_with(r'bool\s+seen\[9\]', src).get('common.h') == 1
    assert _elsewhere(r'\bseen\[', src) == {}
    # the tap table relative to the origin: filled by segnb_rel_taps
    assert _elsewhere(r'\.d[hw]\[t\]\s*=\s*(\(signed char\))?\(?g->d[hw]\[t\]\s*-', src) == {}
    for name in ('segnb_tap_window', 'segnb_rel_taps', 'segnb_window_once_3x3', 'segnb_nhwc_bytes', 'segnb_fits_desc',
                 'segnb_opt_in_lds', 'whole_output', 'whole_output_3x3_s1', 'segnb_try_launched'):
        assert files_with(r'(?m)^(SEGNB_HOST_INLINE|inline|int)\s[\w ]*\b%s\([^;{]*\)\s*\{' % name, src) == {'common.h': 1}, name
    assert src['common.h'].count('spans are 2') == 1 and _elsewhere(r'spans are 2', src) == {}


def test_lds_opt_in_is_written_once():
    assert files_with(r'hipFuncSetAttribute') == {'common.h': 2}      # (the call and its message)
    assert files_with(r'\bset_smem\b') == {}


def test_one_declined_status():
    src = sources()
    assert files_with(r'-\s*12345\b', src) == {} and files_with(r'NOT_HANDLED', src) == {}
    assert files_with(r'constexpr\s+int\s+SEGNB_LAUNCH_DECLINED\s*=', src) == {'common.h': 1}
    # its only reader is segnb_try_launched: everywhere else the constant is returned, never compared
    assert files_with(r'[!=]=\s*SEGNB_LAUNCH_DECLINED|SEGNB_LAUNCH_DECLINED\s*[!=]=', src) == {'common.h': 1}
    for name, text in src.items():
        if name != 'common.h':
            assert len(re.findall(r'SEGNB_LAUNCH_DECLINED', text)) == len(re.findall(r'return SEGNB_LAUNCH_DECLINED;', text)), name


def test_descriptor_extent_is_written_once():
    src = sources()
    # ((pixels - 1) * ld + C) * element size, under any operand names; and its comparison with 2 GiB
    assert _elsewhere(r'-\s*1\)\s*\*\s*[\w.\->]+\s*\+\s*[\w.\->]+\)\s*\*\s*(2|4|esz)\b', src) == {}
    assert len(re.findall(r'-\s*1\)\s*\*\s*ld\s*\+\s*C\)\s*\*\s*esz', src['common.h'])) == 1
    # what is still compared with 1ll << 31 elsewhere is a pixel count, a weight matrix or a workspace -- other statements
    for name, text in src.items():
        for line in text.split('\n'):
            if '1ll << 31' in line and name != 'common.h':
                assert re.search(r'N \* (g->)?H|\bw\b|\bwb\b|tiles \* ks|N \* g->Hi', line), (name, line)


def test_whole_output_gate_is_written_once():
    src = sources()
    assert _elsewhere(r'out_step\s*[!=]=\s*1', src) == {}
    assert _elsewhere(r'QH\s*[!=]=\s*g->Ho', src) == {}
    assert len(re.findall(r'QH\s*==\s*g->Ho', src['common.h'])) == 1
