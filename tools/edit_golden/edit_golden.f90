!==========================================================================!
! edit_golden: the reference's set_value / add_value / get_value /          !
! set_multiple_values / add_multiple_values / add_sparse_matrix /           !
! scalar_multiply / zero on one CSR or ELLPACK matrix, for the fixtures     !
! under tests/golden/edit.  Only `use`s the reference's modules; compiled   !
! against the objects and .mod files of oracle/build_ref.sh (see            !
! make_fixtures.py).                                                        !
!                                                                           !
!   edit_golden in.bin out.bin                                              !
! in.bin (stream, native endian): int32 fmt (0 csr, 1 ellpack), nrow, ncol, !
!   ne, ei(ne), ej(ne): the pattern, assembled the reference's way          !
!   (ll_graph%add_edge in order, convert_graph_type, set_graph, zero).      !
!   Then operations, each an int32 code and its arguments:                  !
!   1 set_value batch   m, i(m), j(m), real64 z(m)  (one call per triple)   !
!   2 add_value batch   the same                                            !
!   3 add_multiple_values  ni, nj, is(ni), js(nj), real64 B(ni,nj)          !
!   4 set_multiple_values  the same                                         !
!   5 add_sparse_matrix has_alpha, real64 alpha, bfmt, bne, bi, bj, bv      !
!   6 scalar_multiply   real64 alpha                                        !
!   7 zero                                                                  !
!   8 get_value batch   m, i(m), j(m)                                       !
!   0 end                                                                   !
! out.bin: the structure as the reference holds it (csr: nnz, ptr, node;    !
!   ellpack: max_d, node(max_d,n), degrees), then after every operation the !
!   whole value array (operation 8: the m values read instead; operation 5: !
!   B's structure and values first).                                        !
!==========================================================================!
program edit_golden
use types, only: dp
use graphs
use sparse_matrices
implicit none
    character(len=512) :: fin, fout
    integer :: u, v, fmt, nrow, ncol, code, m, k, l, ni, nj, has_alpha, bfmt
    integer, allocatable :: is(:), js(:)
    real(dp), allocatable :: z(:), B(:,:)
    real(dp) :: alpha
    class(sparse_matrix_interface), pointer :: A, Bm

    call get_command_argument(1, fin)
    call get_command_argument(2, fout)
    open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
    open(newunit=v, file=trim(fout), access='stream', form='unformatted', status='replace')
    read(u) fmt, nrow, ncol
    call read_pattern(u, fmt, nrow, ncol, A, .false.)
    call write_structure(v, A)

    do
        read(u) code
        if (code == 0) exit
        select case (code)
        case (1, 2, 8)
            read(u) m
            if (allocated(is)) deallocate(is, js)
            if (allocated(z)) deallocate(z)
            allocate(is(m), js(m), z(m))
            if (m > 0) read(u) is, js
            if (code /= 8 .and. m > 0) read(u) z
            do k = 1, m
                if (code == 1) call A%set_value(is(k), js(k), z(k))
                if (code == 2) call A%add_value(is(k), js(k), z(k))
                if (code == 8) z(k) = A%get_value(is(k), js(k))
            enddo
            if (code == 8) write(v) z
        case (3, 4)
            read(u) ni, nj
            if (allocated(is)) deallocate(is, js)
            if (allocated(B)) deallocate(B)
            allocate(is(ni), js(nj), B(ni, nj))
            read(u) is, js, B
            if (code == 3) call A%add_multiple_values(is, js, B)
            if (code == 4) call A%set_multiple_values(is, js, B)
        case (5)
            read(u) has_alpha, alpha, bfmt
            call read_pattern(u, bfmt, nrow, ncol, Bm, .true.)
            call write_structure(v, Bm)
            call write_values(v, Bm)
            if (has_alpha /= 0) then
                call A%add_sparse_matrix(Bm, alpha)
            else
                call A%add_sparse_matrix(Bm)
            endif
        case (6)
            read(u) alpha
            call A%scalar_multiply(alpha)
        case (7)
            call A%zero()
        end select
        if (code /= 8) call write_values(v, A)
    enddo
    close(u)
    close(v)

contains

subroutine read_pattern(u, fmt, nrow, ncol, M, with_values)
    integer, intent(in) :: u, fmt, nrow, ncol
    class(sparse_matrix_interface), pointer, intent(out) :: M
    logical, intent(in) :: with_values
    integer :: ne, k
    integer, allocatable :: ei(:), ej(:)
    real(dp), allocatable :: ev(:)
    class(graph_interface), pointer :: g

    read(u) ne
    allocate(ei(ne), ej(ne), ev(ne))
    if (ne > 0) read(u) ei, ej
    if (with_values .and. ne > 0) read(u) ev
    allocate(ll_graph :: g)
    call g%init(nrow, ncol)
    do k = 1, ne
        call g%add_edge(ei(k), ej(k))
    enddo
    if (fmt == 0) then
        call convert_graph_type(g, "compressed sparse")
        allocate(csr_matrix :: M)
    else
        call convert_graph_type(g, "ellpack")
        allocate(ellpack_matrix :: M)
    endif
    call M%init(nrow, ncol)
    call M%set_graph(g)
    call M%zero()
    if (with_values) then
        do k = 1, ne
            call M%set_value(ei(k), ej(k), ev(k))
        enddo
    endif
end subroutine

subroutine write_structure(v, M)
    integer, intent(in) :: v
    class(sparse_matrix_interface), intent(in) :: M
    select type (M)
    type is (csr_matrix)
        write(v) size(M%g%node), M%g%ptr, M%g%node
    type is (ellpack_matrix)
        write(v) M%g%max_d, M%g%node, M%g%degrees
    end select
end subroutine

subroutine write_values(v, M)
    integer, intent(in) :: v
    class(sparse_matrix_interface), intent(in) :: M
    select type (M)
    type is (csr_matrix)
        write(v) M%val
    type is (ellpack_matrix)
        write(v) M%val
    end select
end subroutine

end program edit_golden
