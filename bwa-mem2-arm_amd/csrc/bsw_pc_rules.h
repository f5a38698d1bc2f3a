// bsw_pc_rules.h -- the tunables of the packed-column kernel's row-level rules (bsw_pc.hip; DESIGN.md §3
// items 10-13): on / off switches and schedule constants, nothing else.  Read by the kernel and, as plain C,
// by the CPU model of the kernel's loop (tests/pc_wave_model.c), so the two cannot drift apart.  Every value
// can be overridden from the command line for a same-box A/B build (make ab AB_FLAGS=-DBSW_PC_RP_MARGIN=24).
#ifndef BSW_PC_RULES_H
#define BSW_PC_RULES_H

// ---- early stop (§3 item 10)
//   BSW_PC_EARLY_STOP 0 : off (the literal loop)
//   BSW_PC_EARLY_SCAN 0 : the scalar bound only, no per-cell scan
#ifndef BSW_PC_EARLY_STOP
#define BSW_PC_EARLY_STOP 1
#endif
#ifndef BSW_PC_EARLY_SCAN
#define BSW_PC_EARLY_SCAN 1
#endif
// rows on which a lane may ask for the scan: (i & BSW_PC_SCAN_PHASE) == BSW_PC_SCAN_PHASE, a
// wave-uniform test (3: every fourth row; 0, 1, 7 and 15 measured in DESIGN.md §4.5)
#ifndef BSW_PC_SCAN_PHASE
#define BSW_PC_SCAN_PHASE 3
#endif

// ---- left skip (§3 item 11)
//   BSW_PC_LEFT_SKIP 0 : off
//   BSW_PC_SKIP_MASK, BSW_PC_SKIP_ROW : gz is refreshed at the end of rows with (i & MASK) == ROW
//   BSW_PC_SKIP_QMIN   : the smallest QMAX class that carries the skip (the classes below it would
//                        pay for gz and the walk with a wave per SIMD)
#ifndef BSW_PC_LEFT_SKIP
#define BSW_PC_LEFT_SKIP 1
#endif
#ifndef BSW_PC_SKIP_MASK
#define BSW_PC_SKIP_MASK 3
#endif
#ifndef BSW_PC_SKIP_ROW
#define BSW_PC_SKIP_ROW 1
#endif
#ifndef BSW_PC_SKIP_QMIN
#define BSW_PC_SKIP_QMIN 96
#endif

// ---- left prune (§3 item 12)
//   BSW_PC_LEFT_PRUNE 0 : off, the walk of item 11 alone
//   BSW_PC_PRUNE_QMIN   : the smallest QMAX class that carries it.  The byte planes never do: the rule's
//                        state costs them scratch (QMAX 128, 160) or a wave per SIMD (96), as it costs the
//                        int16 96 class its third wave (168 -> 175 VGPRs)
#ifndef BSW_PC_LEFT_PRUNE
#define BSW_PC_LEFT_PRUNE 1
#endif
#ifndef BSW_PC_PRUNE_QMIN
#define BSW_PC_PRUNE_QMIN 128
#endif

// ---- right prune (§3 item 13; the sweep behind the values: profiles/right_prune/ab.txt)
//   BSW_PC_RIGHT_PRUNE 0 : off; on, it runs in the classes of BSW_PC_PRUNE_QMIN
//   MARGIN : T = best - MARGIN, the threshold a cell's bound is held against
//   SLACK, SLACK2 : the zeroing test's and the soft retreat's distance from T
//   K      : the rows since a staying lane's last new best that the precheck allows
//   ROW0   : the first row on which the precheck allows a cap
#ifndef BSW_PC_RIGHT_PRUNE
#define BSW_PC_RIGHT_PRUNE 1
#endif
#ifndef BSW_PC_RP_MARGIN
#define BSW_PC_RP_MARGIN 20
#endif
#ifndef BSW_PC_RP_SLACK
#define BSW_PC_RP_SLACK 12
#endif
#ifndef BSW_PC_RP_SLACK2
#define BSW_PC_RP_SLACK2 11
#endif
#ifndef BSW_PC_RP_K
#define BSW_PC_RP_K 16
#endif
#ifndef BSW_PC_RP_WALK_MASK        // a marked wave walks on refresh rows with (i & MASK) == (BSW_PC_SKIP_ROW & MASK)
#define BSW_PC_RP_WALK_MASK 15
#endif
#ifndef BSW_PC_RP_RWIN             // the retreat looks at lanes whose band end is within RWIN slots of the cap
#define BSW_PC_RP_RWIN 4
#endif
#ifndef BSW_PC_RP_ROW0
#define BSW_PC_RP_ROW0 25
#endif

#endif  // BSW_PC_RULES_H
