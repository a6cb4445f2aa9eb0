"""The calls of tests/test_train_entry_refusals.py and of its recorder tests/golden/make_train_entry_refusals.py: for every C entry of the
training operators (csrc/*_train.hip), its arguments in the order of include/daspeech_decode.h and the calls that the argument gates answer
before any device call — a refusal (rc < 0, with its message), or DSP_OK on the "nothing to do" path.

The pointers are made-up addresses that nothing ever reads: a(i) lies on the 16-byte grid, a(i) + 2 off it.  A case is (name, {argument:
value}) over the entry's BASE; ok=True marks the calls that return DSP_OK.  Every case was walked through its entry's gates by hand: none
may reach a launch (the recorder refuses to record a call that returns anything but its refusal or its DSP_OK).  Entries with a `_state`
twin (daspeech_amd._lib.STATE_ENTRIES) run every case on both, the twin with an aligned rng_state, and the twin alone gets STATE_CASES.
"""
BIG = 1 << 40           # workspace_bytes no entry asks more than
THR_OVER = (1 << 24) + 1


def a(i):
    return 0x10000000 + 0x1000 * i


RNG = a(40)
STATE_CASES = [("rng_state at +4 bytes", {"rng_state": RNG + 4})]


def ws_cases(ws):
    return [("null workspace", {"workspace": None}), ("short workspace", {"workspace_bytes": 0}), ("workspace at +2 bytes", {"workspace": ws + 2})]


ENTRIES = {}


def entry(name, base, cases, ok=()):
    ENTRIES[name] = {"base": base, "cases": cases, "ok": list(ok)}


# ---------------------------------------------------------------- act_dropout_train.hip
entry("dsp_act_dropout_train_fwd",
      [("h", a(0)), ("ld_h", 72), ("bias", a(1)), ("act", 3), ("keep_scale", 1.0), ("thr", 0), ("seed", 0), ("offset", 0), ("y", a(2)),
       ("act_dtype", 1), ("param_dtype", 0), ("R", 37), ("Cin", 72)],
      [("null h", {"h": None}), ("null y", {"y": None}), ("y is h", {"y": a(0)}), ("bias is y", {"bias": a(2)}),
       ("h at +2 bytes", {"h": a(0) + 2}), ("bias at +2 bytes", {"bias": a(1) + 2}), ("y at +2 bytes", {"y": a(2) + 2}),
       ("thr above 2^24", {"thr": THR_OVER}), ("Cin off the vector", {"Cin": 70})],
      ok=[("no rows", {"R": 0})])
entry("dsp_act_dropout_train_bwd",
      [("dy", a(0)), ("h", a(1)), ("ld_h", 72), ("bias", a(2)), ("act", 3), ("keep_scale", 1.0), ("thr", 0), ("seed", 0), ("offset", 0),
       ("dh", a(3)), ("dbias", a(4)), ("workspace", a(5)), ("workspace_bytes", BIG), ("act_dtype", 1), ("param_dtype", 0), ("R", 37), ("Cin", 72)],
      [("null dy", {"dy": None}), ("null h", {"h": None}), ("dh is dy", {"dh": a(0)}), ("dh is dbias", {"dh": a(4)}), ("dbias is h", {"dbias": a(1)}),
       ("dy at +2 bytes", {"dy": a(0) + 2}), ("dbias at +2 bytes", {"dbias": a(4) + 2})] + ws_cases(a(5)),
      ok=[("no rows", {"R": 0}), ("no gradient asked for", {"dh": None, "dbias": None})])

# ---------------------------------------------------------------- residual_norm_train.hip
entry("dsp_resnorm_train_fwd",
      [("h", a(0)), ("residual", a(1)), ("bias", a(2)), ("gamma", a(3)), ("beta", a(4)), ("eps", 1e-5), ("alpha", 1.0), ("keep_scale", 1.0), ("thr", 0),
       ("seed", 0), ("offset", 0), ("s", a(5)), ("y", a(6)), ("stats", a(7)), ("act_dtype", 1), ("param_dtype", 0), ("R", 37), ("C", 72)],
      [("null residual", {"residual": None}), ("null stats", {"stats": None}), ("h without s", {"s": None}), ("y is residual", {"y": a(1)}),
       ("s is y", {"s": a(6)}), ("h at +2 bytes", {"h": a(0) + 2}), ("gamma at +2 bytes", {"gamma": a(3) + 2}), ("stats at +4 bytes", {"stats": a(7) + 4}),
       ("thr above 2^24", {"thr": THR_OVER})],
      ok=[("no rows", {"R": 0})])
entry("dsp_resnorm_train_bwd",
      [("dy", a(0)), ("ds", a(1)), ("s", a(2)), ("stats", a(3)), ("gamma", a(4)), ("alpha", 1.0), ("keep_scale", 1.0), ("thr", 0), ("seed", 0), ("offset", 0),
       ("dh", a(5)), ("dresidual", a(6)), ("dbias", a(7)), ("dgamma", a(8)), ("dbeta", a(9)), ("workspace", a(10)), ("workspace_bytes", BIG),
       ("act_dtype", 1), ("param_dtype", 0), ("R", 37), ("C", 72)],
      [("dy without s", {"s": None}), ("dh is dy", {"dh": a(0)}), ("dh is dresidual", {"dh": a(6)}), ("dresidual is s", {"dresidual": a(2)}),
       ("dy at +2 bytes", {"dy": a(0) + 2}), ("dh at +2 bytes", {"dh": a(5) + 2}), ("stats at +4 bytes", {"stats": a(3) + 4}),
       ("thr above 2^24", {"thr": THR_OVER})] + ws_cases(a(10)),
      ok=[("no rows", {"R": 0}), ("no gradient asked for", {"dh": None, "dresidual": None, "dbias": None, "dgamma": None, "dbeta": None})])
entry("dsp_dropout_keep_mask",
      [("seed", 0), ("offset", 0), ("thr", 0), ("out", a(0)), ("n", 64)],
      [("null out", {"out": None}), ("negative n", {"n": -1}), ("thr above 2^24", {"thr": THR_OVER})],
      ok=[("no elements", {"n": 0})])
entry("dsp_dropout_state_advance",
      [("rng_state", RNG), ("by", 4)],
      [("null rng_state", {"rng_state": None}), ("rng_state at +4 bytes", {"rng_state": RNG + 4})])

# ---------------------------------------------------------------- conformer_train.hip
entry("dsp_dwconv_bn_silu_train_fwd",
      [("x", a(0)), ("w", a(1)), ("gamma", a(2)), ("beta", a(3)), ("running_mean", a(4)), ("running_var", a(5)), ("momentum", 0.1), ("eps", 1e-5),
       ("y", a(6)), ("save_mean", a(7)), ("save_invstd", a(8)), ("workspace", a(9)), ("workspace_bytes", BIG), ("act_dtype", 1), ("bn_dtype", 0),
       ("B", 2), ("T", 100), ("C", 72), ("K", 7)],
      [("null x", {"x": None}), ("null save_mean", {"save_mean": None}), ("y is x", {"y": a(0)}), ("save_mean is save_invstd", {"save_mean": a(8)}),
       ("x at +2 bytes", {"x": a(0) + 2}), ("y at +2 bytes", {"y": a(6) + 2}), ("one frame", {"B": 1, "T": 1}), ("K = 5", {"K": 5})] + ws_cases(a(9)),
      ok=[("no samples", {"B": 0})])
entry("dsp_dwconv_bn_silu_train_bwd",
      [("x", a(0)), ("w", a(1)), ("gamma", a(2)), ("beta", a(3)), ("save_mean", a(4)), ("save_invstd", a(5)), ("grad_y", a(6)), ("dx", a(7)), ("dw", a(8)),
       ("dgamma", a(9)), ("dbeta", a(10)), ("workspace", a(11)), ("workspace_bytes", BIG), ("act_dtype", 1), ("bn_dtype", 0), ("B", 2), ("T", 100),
       ("C", 72), ("K", 7)],
      [("null grad_y", {"grad_y": None}), ("dx is x", {"dx": a(0)}), ("dx is grad_y", {"dx": a(6)}), ("dw is w", {"dw": a(1)}),
       ("x at +2 bytes", {"x": a(0) + 2}), ("grad_y at +2 bytes", {"grad_y": a(6) + 2}), ("dx at +2 bytes", {"dx": a(7) + 2})] + ws_cases(a(11)),
      ok=[("no samples", {"B": 0}), ("no gradient asked for", {"dx": None, "dw": None, "dgamma": None, "dbeta": None})])

# ---------------------------------------------------------------- conv1d_train.hip, conv1d_stride2_train.hip
for _name, _cin, _bad_cin in (("dsp_conv1d_train", 64, 32), ("dsp_conv1d_s2_train", 16, 8)):
    _size_cases = [("fp32 data", {"act_dtype": 0}), ("bias dtype", {"bias_dtype": 2}), ("Cin off the granule", {"Cin": _bad_cin}), ("Cout = 80", {"Cout": 80}),
                   ("K even", {"K": 4}), ("K = 17", {"K": 17}), ("T = 0", {"T": 0}), ("negative B", {"B": -1})]
    entry(_name + "_fwd",
          [("x", a(0)), ("ld_x", _cin), ("w", a(1)), ("bias", a(2)), ("y", a(3)), ("ld_y", 64), ("workspace", a(4)), ("workspace_bytes", BIG),
           ("act_dtype", 1), ("bias_dtype", 0), ("B", 2), ("T", 9), ("Cin", _cin), ("Cout", 64), ("K", 3)],
          [("null x", {"x": None}), ("null w", {"w": None}), ("null y", {"y": None}), ("y is x", {"y": a(0)}), ("y is bias", {"y": a(2)}),
           ("workspace is x", {"workspace": a(0)}), ("workspace is bias", {"workspace": a(2)}), ("x at +2 bytes", {"x": a(0) + 2}),
           ("bias at +2 bytes", {"bias": a(2) + 2}), ("y at +2 bytes", {"y": a(3) + 2}), ("ld_x off the 8-element grid", {"ld_x": _cin + 4}),
           ("ld_y below Cout", {"ld_y": 56})] + _size_cases + ws_cases(a(4)),
          ok=[("no samples", {"B": 0})])
    entry(_name + "_bwd",
          [("dy", a(0)), ("ld_dy", 64), ("x", a(1)), ("ld_x", _cin), ("w", a(2)), ("dx", a(3)), ("dw", a(4)), ("db", a(5)), ("workspace", a(6)),
           ("workspace_bytes", BIG), ("act_dtype", 1), ("bias_dtype", 0), ("B", 2), ("T", 9), ("Cin", _cin), ("Cout", 64), ("K", 3)],
          [("null dy", {"dy": None}), ("null w", {"w": None}), ("dx is x", {"dx": a(1)}), ("dw is the workspace", {"dw": a(6)}), ("dx is dw", {"dx": a(4)}),
           ("dw is db", {"dw": a(5)}), ("workspace is x", {"workspace": a(1)}), ("dy at +2 bytes", {"dy": a(0) + 2}), ("db at +2 bytes", {"db": a(5) + 2}),
           ("ld_dy off the 8-element grid", {"ld_dy": 68})] + _size_cases + ws_cases(a(6)),
          ok=[("no samples", {"B": 0}), ("no gradient asked for", {"dx": None, "dw": None, "db": None, "workspace": None, "workspace_bytes": 0})])

# ---------------------------------------------------------------- mha_train.hip
entry("dsp_mha_train_fwd",
      [("q", a(0)), ("ldq", 64), ("k", a(1)), ("v", a(2)), ("ldkv", 64), ("pad_mask", None), ("keep_scale", 1.0), ("thr", 0), ("seed", 0), ("offset", 0),
       ("out", a(3)), ("lse", a(4)), ("act_dtype", 1), ("B", 2), ("N", 8), ("M", 8), ("H", 1)],
      [("null q", {"q": None}), ("null lse", {"lse": None}), ("out is q", {"out": a(0)}), ("lse is out", {"lse": a(3)}), ("lse is k", {"lse": a(1)}),
       ("q at +2 bytes", {"q": a(0) + 2}), ("lse at +4 bytes", {"lse": a(4) + 4}), ("thr above 2^24", {"thr": THR_OVER})],
      ok=[("no samples", {"B": 0})])
entry("dsp_mha_train_bwd",
      [("dout", a(0)), ("q", a(1)), ("ldq", 64), ("k", a(2)), ("v", a(3)), ("ldkv", 64), ("pad_mask", None), ("lse", a(4)), ("keep_scale", 1.0), ("thr", 0),
       ("seed", 0), ("offset", 0), ("dq", a(5)), ("dk", a(6)), ("dv", a(7)), ("workspace", a(8)), ("workspace_bytes", BIG), ("act_dtype", 1), ("B", 2),
       ("N", 8), ("M", 8), ("H", 1)],
      [("null dout", {"dout": None}), ("null lse", {"lse": None}), ("dq is q", {"dq": a(1)}), ("workspace is q", {"workspace": a(1)}),
       ("dq is dk", {"dq": a(6)}), ("dk is the workspace", {"dk": a(8)}), ("dout at +2 bytes", {"dout": a(0) + 2}), ("dv at +2 bytes", {"dv": a(7) + 2})]
      + ws_cases(a(8)),
      ok=[("no samples", {"B": 0}), ("no gradient asked for", {"dq": None, "dk": None, "dv": None})])

# ---------------------------------------------------------------- relpos_attention_train.hip
entry("dsp_relpos_attention_train_fwd",
      [("q", a(0)), ("k", a(1)), ("v", a(2)), ("ld", 64), ("pos", a(3)), ("bias_u", a(4)), ("bias_v", a(5)), ("pad_mask", None), ("keep_scale", 1.0), ("thr", 0),
       ("seed", 0), ("offset", 0), ("out", a(6)), ("lse", a(7)), ("act_dtype", 1), ("param_dtype", 0), ("B", 3), ("T", 40), ("H", 1)],
      [("null q", {"q": None}), ("null bias_u", {"bias_u": None}), ("null lse", {"lse": None}), ("out is q", {"out": a(0)}), ("out is pos", {"out": a(3)}),
       ("q at +2 bytes", {"q": a(0) + 2}), ("lse at +4 bytes", {"lse": a(7) + 4}), ("thr above 2^24", {"thr": THR_OVER})],
      ok=[("no samples", {"B": 0})])
entry("dsp_relpos_attention_train_bwd",
      [("dout", a(0)), ("q", a(1)), ("k", a(2)), ("v", a(3)), ("ld", 64), ("pos", a(4)), ("bias_u", a(5)), ("bias_v", a(6)), ("pad_mask", None), ("out", a(7)),
       ("lse", a(8)), ("keep_scale", 1.0), ("thr", 0), ("seed", 0), ("offset", 0), ("dq", a(9)), ("dk", a(10)), ("dv", a(11)), ("dpos", a(12)),
       ("dbias_u", a(13)), ("dbias_v", a(14)), ("workspace", a(15)), ("workspace_bytes", BIG), ("act_dtype", 1), ("param_dtype", 0), ("B", 3), ("T", 40),
       ("H", 1)],
      [("null dout", {"dout": None}), ("null out", {"out": None}), ("dq is q", {"dq": a(1)}), ("dbias_v is lse", {"dbias_v": a(8)}),
       ("dpos is dbias_u", {"dpos": a(13)}), ("dq is dk", {"dq": a(10)}), ("dout at +2 bytes", {"dout": a(0) + 2}), ("dbias_v at +2 bytes", {"dbias_v": a(14) + 2}),
       ("thr above 2^24", {"thr": THR_OVER})] + ws_cases(a(15)),
      ok=[("no samples", {"B": 0}),
          ("no gradient asked for", {"dq": None, "dk": None, "dv": None, "dpos": None, "dbias_u": None, "dbias_v": None})])

# ---------------------------------------------------------------- embed_entry_train.hip
entry("dsp_embed_entry_fwd",
      [("tokens", a(0)), ("ld_tok", 8), ("E", a(1)), ("P", a(2)), ("pad", 1), ("embed_scale", 1.0), ("keep_scale", 1.0), ("thr", 0), ("seed", 0), ("offset", 0),
       ("y", a(3)), ("tok32", a(4)), ("pos32", a(5)), ("dtype", 1), ("B", 2), ("L", 8), ("V", 100), ("NP", 20), ("C", 64)],
      [("null tokens", {"tokens": None}), ("null pos32", {"pos32": None}), ("y is E", {"y": a(1)}), ("y is P", {"y": a(2)}), ("E at +2 bytes", {"E": a(1) + 2}),
       ("tokens at +4 bytes", {"tokens": a(0) + 4}), ("tok32 at +2 bytes", {"tok32": a(4) + 2}), ("ld_tok below L", {"ld_tok": 7}), ("negative L", {"L": -1})],
      ok=[("no samples", {"B": 0})])
entry("dsp_embed_entry_bwd",
      [("dy", a(0)), ("tok32", a(1)), ("pos32", a(2)), ("pad", 1), ("embed_scale", 1.0), ("keep_scale", 1.0), ("thr", 0), ("seed", 0), ("offset", 0),
       ("dE", a(3)), ("dP", a(4)), ("workspace", a(5)), ("workspace_bytes", BIG), ("dtype", 1), ("n", 16), ("V", 100), ("NP", 20), ("C", 64)],
      [("null dy", {"dy": None}), ("null tok32", {"tok32": None}), ("dE is dP", {"dE": a(4)}), ("dy is dE", {"dy": a(3)}), ("dy at +2 bytes", {"dy": a(0) + 2}),
       ("dP at +2 bytes", {"dP": a(4) + 2})] + ws_cases(a(5)) + [("short workspace, masked", {"workspace_bytes": 16, "thr": 1 << 23})],
      ok=[("no gradient asked for", {"dE": None, "dP": None}), ("no rows, no gradient asked for", {"n": 0, "dE": None, "dP": None})])
entry("dsp_pos_add_fwd",
      [("x", a(0)), ("ld_x", 64), ("padding_mask", a(1)), ("tab", a(2)), ("alpha", a(3)), ("pad", 1), ("keep_scale", 1.0), ("thr", 0), ("seed", 0), ("offset", 0),
       ("y", a(4)), ("pos32", a(5)), ("act_dtype", 1), ("tab_dtype", 0), ("alpha_dtype", 0), ("B", 2), ("N", 8), ("NT", 50), ("C", 64)],
      [("null x", {"x": None}), ("null alpha", {"alpha": None}), ("y is x", {"y": a(0)}), ("y is tab", {"y": a(2)}), ("x at +2 bytes", {"x": a(0) + 2}),
       ("tab at +2 bytes", {"tab": a(2) + 2}), ("ld_x below C", {"ld_x": 56}), ("negative pad", {"pad": -1})],
      ok=[("no samples", {"B": 0})])
entry("dsp_pos_add_bwd",
      [("dy", a(0)), ("tab", a(1)), ("pos32", a(2)), ("keep_scale", 1.0), ("thr", 0), ("seed", 0), ("offset", 0), ("dx", a(3)), ("dalpha", a(4)),
       ("workspace", a(5)), ("workspace_bytes", BIG), ("act_dtype", 1), ("tab_dtype", 0), ("alpha_dtype", 0), ("R", 16), ("NT", 50), ("C", 64)],
      [("null dy", {"dy": None}), ("dalpha without tab", {"tab": None}), ("dx is dy", {"dx": a(0)}), ("dy at +2 bytes", {"dy": a(0) + 2}),
       ("dx at +2 bytes", {"dx": a(3) + 2})] + ws_cases(a(5)),
      ok=[("no gradient asked for", {"dx": None, "dalpha": None}), ("no rows, no gradient asked for", {"R": 0, "dx": None, "dalpha": None})])

# ---------------------------------------------------------------- tts_loss_train.hip
_TL_IN = [("audio_lens", a(3)), ("log_dur_out", a(4)), ("pitch_out", a(5)), ("energy_out", a(6)), ("durations", a(7)), ("pitches", a(8)), ("energies", a(9)),
          ("src_lens", a(10)), ("len64", 1), ("dur64", 1)]
entry("dsp_tts_loss_fwd",
      [("feat_out", a(0)), ("fo_sb", 640), ("fo_sr", 80), ("feat_post", a(1)), ("fp_sb", 640), ("fp_sr", 80), ("target", a(2)), ("tg_sb", 640), ("tg_sr", 80)]
      + _TL_IN + [("losses", a(11)), ("inv_counts", a(12)), ("workspace", a(13)), ("workspace_bytes", BIG), ("dtype", 1), ("B", 2), ("F_", 8), ("C", 80),
                  ("N", 6)],
      [("null feat_out", {"feat_out": None}), ("null src_lens", {"src_lens": None}), ("null losses", {"losses": None}), ("losses is target", {"losses": a(2)}),
       ("workspace is feat_post", {"workspace": a(1)}), ("losses is inv_counts", {"losses": a(12)}), ("inv_counts is the workspace", {"inv_counts": a(13)}),
       ("feat_out at +1 byte", {"feat_out": a(0) + 1}), ("audio_lens at +4 bytes", {"audio_lens": a(3) + 4}), ("losses at +2 bytes", {"losses": a(11) + 2}),
       ("negative stride", {"tg_sr": -80}), ("no features", {"C": 0})] + ws_cases(a(13)),
      ok=[("no samples", {"B": 0})])
entry("dsp_tts_loss_bwd",
      [("grad_losses", a(20)), ("inv_counts", a(21)), ("feat_out", a(0)), ("fo_sb", 640), ("fo_sr", 80), ("feat_post", a(1)), ("fp_sb", 640), ("fp_sr", 80),
       ("target", a(2)), ("tg_sb", 640), ("tg_sr", 80)] + _TL_IN +
      [("d_feat_out", a(13)), ("d_feat_post", a(14)), ("d_log_dur", a(15)), ("d_pitch", a(16)), ("d_energy", a(17)), ("dtype", 1), ("B", 2), ("F", 8), ("F_", 8),
       ("C", 80), ("N", 6)],
      [("null grad_losses", {"grad_losses": None}), ("null src_lens", {"src_lens": None}), ("d_feat_post without feat_post", {"feat_post": None}),
       ("d_feat_out is feat_out", {"d_feat_out": a(0)}), ("d_energy is feat_post", {"d_energy": a(1)}), ("d_pitch is d_log_dur", {"d_pitch": a(15)}),
       ("d_energy at +1 byte", {"d_energy": a(17) + 1}), ("grad_losses at +2 bytes", {"grad_losses": a(20) + 2}), ("F_ above F", {"F_": 9})],
      ok=[("no samples", {"B": 0}),
          ("no gradient asked for", {"d_feat_out": None, "d_feat_post": None, "d_log_dur": None, "d_pitch": None, "d_energy": None})])

# ---------------------------------------------------------------- path_features_train.hip
entry("dsp_path_features_fwd",
      [("features", a(0)), ("ld_f", 64), ("path", a(1)), ("path_sb", 10), ("path_sc", 1), ("path64", 1), ("skip_first", 0), ("out", a(2)), ("pad", a(3)),
       ("n", a(4)), ("dtype", 1), ("B", 2), ("L", 10), ("W", 6), ("C", 64)],
      [("null features", {"features": None}), ("null n", {"n": None}), ("out is features", {"out": a(0)}), ("features at +2 bytes", {"features": a(0) + 2}),
       ("n at +4 bytes", {"n": a(4) + 4}), ("null path", {"path": None}), ("path at +4 bytes", {"path": a(1) + 4}), ("ld_f below C", {"ld_f": 56})],
      ok=[("no samples", {"B": 0}), ("no output rows", {"W": 0})])
entry("dsp_path_features_bwd",
      [("dy", a(0)), ("dy_sb", 384), ("dy_sr", 64), ("path", a(1)), ("path_sb", 10), ("path_sc", 1), ("path64", 1), ("skip_first", 0), ("dfeatures", a(2)),
       ("dtype", 1), ("B", 2), ("L", 10), ("W", 6), ("C", 64)],
      [("null dfeatures", {"dfeatures": None}), ("dfeatures is dy", {"dfeatures": a(0)}), ("dfeatures at +2 bytes", {"dfeatures": a(2) + 2}),
       ("null dy", {"dy": None}), ("dy at +2 bytes", {"dy": a(0) + 2}), ("dy_sr off the vector", {"dy_sr": 60}), ("null path", {"path": None})],
      ok=[("no samples", {"B": 0})])


def calls():
    """Every call as (entry, case, expects DSP_OK, [argument values in C order, the stream last])."""
    from daspeech_amd._lib import STATE_ENTRIES
    out = []
    for name, e in ENTRIES.items():
        twins = [(name, [])] + ([(name + "_state", [("rng_state", RNG)])] if name in STATE_ENTRIES else [])
        for sym, extra in twins:
            base = e["base"] + extra
            keys = [k for k, _ in base]
            todo = [(c, o, False) for c, o in e["cases"]] + [(c, o, True) for c, o in e["ok"]] + ([(c, o, False) for c, o in STATE_CASES] if extra else [])
            for case, over, ok in todo:
                assert set(over) <= set(keys), (sym, case)
                args = dict(base)
                args.update(over)
                out.append((sym, case, ok, [args[k] for k in keys] + [None]))
    assert len({(s, c) for s, c, _, _ in out}) == len(out)
    return out
