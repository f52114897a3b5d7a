/* rebase_smoke — oaz_tree_rebase_host from a plain C program, built with -fsanitize=address,undefined against a
 * host-only object of csrc/oaz_tree_rebase.cpp (tests/test_tree_reuse.py): a handful of hand-built trees, one
 * whose children block starts in the same 64-node chunk as its parent, blocks that cross a chunk border, an
 * expanded node without children, and the error cases, which must write nothing. Exits 0 when all hold. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "onitama_az.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c);      \
            exit(1);                                                    \
        }                                                               \
    } while (0)

enum { EXPANDED = 1, TERMINAL = 2 };

/* node i: N visits, W = i + 0.5, P = 1 / (i + 2), mv = 100 + i, not expanded */
static void leaf(oaz_node* t, int i, unsigned N) {
    memset(&t[i], 0, sizeof(t[i]));
    t[i].W = i + 0.5;
    t[i].P = 1.0 / (i + 2);
    t[i].N = N;
    t[i].mv = (uint16_t)(100 + i);
}
static void expand(oaz_node* t, int i, unsigned first, unsigned nch) {
    t[i].first = first;
    t[i].nch = (uint8_t)nch;
    t[i].flags |= EXPANDED;
}
/* everything but `first` of out[j] is in[i]'s (the new root's P and mv aside) */
static void same_node(const oaz_node* out, int j, const oaz_node* in, int i) {
    CHECK(out[j].W == in[i].W && out[j].N == in[i].N && out[j].nch == in[i].nch && out[j].flags == in[i].flags);
    CHECK(out[j].pad == 0);
    if (j == 0) CHECK(out[j].P == 1.0 && out[j].mv == 0);
    else CHECK(out[j].P == in[i].P && out[j].mv == in[i].mv);
}

int main(void) {
    enum { CAP = 256 };
    oaz_node in[CAP], out[CAP], blank[CAP];
    int n = 0, i;
    memset(blank, 0xAB, sizeof(blank));

    /* 1. small: root -> {1, 2, 3}; 2 -> {4, 5} (the block in its parent's chunk); 4 -> {6, 7, 8}; 3 -> {9} */
    for (i = 0; i < 10; ++i) leaf(in, i, (unsigned)(i + 1));
    expand(in, 0, 1, 3);
    expand(in, 2, 4, 2);
    expand(in, 4, 6, 3);
    expand(in, 3, 9, 1);
    memcpy(out, blank, sizeof(out));
    CHECK(oaz_tree_rebase_host(in, 10, 1, out, CAP, &n) == 0 && n == 6);
    {
        const int from[6] = {2, 4, 5, 6, 7, 8};
        for (i = 0; i < 6; ++i) same_node(out, i, in, from[i]);
        CHECK(out[0].first == 1 && out[1].first == 3);
        CHECK(memcmp(&out[6], blank, sizeof(oaz_node)) == 0);
    }
    /* the subtree of child 2 (node 3): {3, 9} */
    CHECK(oaz_tree_rebase_host(in, 10, 2, out, CAP, &n) == 0 && n == 2);
    same_node(out, 0, in, 3);
    same_node(out, 1, in, 9);
    CHECK(out[0].first == 1);
    /* a visited child that was never expanded: a one-node tree */
    CHECK(oaz_tree_rebase_host(in, 10, 0, out, CAP, &n) == 0 && n == 1);
    same_node(out, 0, in, 1);

    /* 2. across chunks: root -> 1..40; 40 -> 41..80 (crosses the first chunk border); 63 -> 81..83 (its block in
     * the next chunk); 64 -> 84..123 (crosses the second border); 100 expanded without a child (first = 124, the
     * node count when it was expanded); 5 -> 124..126 (not in node 40's subtree) */
    for (i = 0; i < 127; ++i) leaf(in, i, 1);
    expand(in, 0, 1, 40);
    expand(in, 40, 41, 40);
    expand(in, 63, 81, 3);
    expand(in, 64, 84, 40);
    expand(in, 100, 124, 0);
    expand(in, 5, 124, 3);
    memcpy(out, blank, sizeof(out));
    CHECK(oaz_tree_rebase_host(in, 127, 39, out, CAP, &n) == 0 && n == 1 + 40 + 3 + 40);
    same_node(out, 0, in, 40);
    for (i = 1; i < n; ++i) same_node(out, i, in, 40 + i); /* nodes 40..123 are all members, in order */
    CHECK(out[0].first == 1 && out[63 - 40].first == 81 - 40 && out[64 - 40].first == 84 - 40);
    CHECK(out[100 - 40].first == (unsigned)n); /* the childless node's first: the node count of the fresh search */
    CHECK(memcmp(&out[n], blank, sizeof(oaz_node)) == 0);
    /* child 4 (node 5): {5, 124, 125, 126} */
    CHECK(oaz_tree_rebase_host(in, 127, 4, out, CAP, &n) == 0 && n == 4);
    same_node(out, 0, in, 5);
    for (i = 1; i < 4; ++i) same_node(out, i, in, 123 + i);
    CHECK(out[0].first == 1);
    /* an exact fit */
    CHECK(oaz_tree_rebase_host(in, 127, 39, out, 84, &n) == 0 && n == 84);

    /* 3. errors write nothing */
    memcpy(out, blank, sizeof(out));
    n = -7;
    leaf(in, 0, 1);
    CHECK(oaz_tree_rebase_host(in, 1, 0, out, CAP, &n) == OAZ_ERR_ARG); /* a one-node tree has no child */
    for (i = 0; i < 127; ++i) leaf(in, i, 1);
    expand(in, 0, 1, 40);
    expand(in, 40, 41, 40);
    in[7].N = 0;
    CHECK(oaz_tree_rebase_host(in, 127, 40, out, CAP, &n) == OAZ_ERR_ARG);  /* out of range */
    CHECK(oaz_tree_rebase_host(in, 127, -1, out, CAP, &n) == OAZ_ERR_ARG);
    CHECK(oaz_tree_rebase_host(in, 127, 6, out, CAP, &n) == OAZ_ERR_ARG);   /* unvisited (node 7) */
    CHECK(oaz_tree_rebase_host(in, 127, 39, out, 40, &n) == OAZ_ERR_CAPACITY); /* 41 nodes */
    CHECK(oaz_tree_rebase_host(in, 0, 0, out, CAP, &n) == OAZ_ERR_ARG);
    CHECK(oaz_tree_rebase_host(NULL, 5, 0, out, CAP, &n) == OAZ_ERR_ARG);
    expand(in, 41, 120, 40); /* a block that leaves the tree */
    CHECK(oaz_tree_rebase_host(in, 127, 39, out, CAP, &n) == OAZ_ERR_ARG);
    CHECK(n == -7 && memcmp(out, blank, sizeof(out)) == 0);
    puts("OK rebase");
    return 0;
}
